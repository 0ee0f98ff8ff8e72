"""Measurement for the inference API (aldi_amd/predictor.py, tta.py, postprocess.py, csrc/infer.hip).  Prints ONE JSON line and writes it
to --out (default profiles/bench_predict.json):

* `Predictor` images/s and ms/image from raw 1024 x 2048 uint8 frames resident in HBM at the reference's INPUT.MIN_SIZE_TEST 1024 /
  MAX_SIZE_TEST 2048 (R50-FPN of configs/cityscapes/ALDI-Best-Cityscapes.yaml, synthetic weights), one image per call: a host clock
  around calls that end in the count's device -> host read;
* device time per call of aldi_detector_postprocess (N = 2, D = 100) and aldi_tta_merge (B = 1, A = 18, D = 100, K = 8, topk 100), from
  device events around 200 back-to-back calls, i.e. the rate of the whole call, not a kernel time;
* test-time augmentation ms/image at the default nine TEST.AUG.MIN_SIZES with flip (18 views, groups of three) from a 480 x 640 frame, and
  its ratio to the ms/image of one plain `Predictor` call on that frame in the same run.  (A 1024 x 2048 frame cannot take the default
  sizes: its 1100 x 2200 and 1200 x 2400 views have more than the 512K anchors per image aldi_rpn_proposals accepts.)

Recorded, not gated."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from aldi_amd import ops
from aldi_amd.postprocess import box_tfm, upload_tfms


def _cfg():
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SEED", 1, "INPUT.MIN_SIZE_TEST", 1024, "INPUT.MAX_SIZE_TEST", 2048])
    return cfg


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernel_us(reps=200):
    g = torch.Generator().manual_seed(0)
    dev = "cuda"

    def dets(*lead):
        x1, y1 = torch.rand(*lead, generator=g) * 1800, torch.rand(*lead, generator=g) * 900
        b = torch.stack([x1, y1, x1 + 20 + torch.rand(*lead, generator=g) * 300, y1 + 20 + torch.rand(*lead, generator=g) * 200], -1)
        return b.to(dev), torch.rand(*lead, generator=g).to(dev), torch.randint(0, 8, lead, generator=g, dtype=torch.int32).to(dev)
    N, D = 2, 100
    b, s, c = dets(N, D)
    cnt = torch.full((N,), D, dtype=torch.int32, device=dev)
    tf = upload_tfms([box_tfm((2048, 1024), (2048 / 1600, 1024 / 800))] * N, dev)
    ob, os_, oc, on = torch.empty_like(b), torch.empty_like(s), torch.empty_like(c), torch.empty_like(cnt)
    post = _events(lambda: ops.detector_postprocess(b, s, c, cnt, tf, ob, os_, oc, on), reps)
    B, A = 1, 18
    b, s, c = dets(B, A, D)
    cnt = torch.full((B, A), D, dtype=torch.int32, device=dev)
    tf = upload_tfms([box_tfm((2048, 1024), (1.0, 1.0), (1.0, 1.0), flip_w=2048 if a % 2 else None) for a in range(A)], dev)
    ws = torch.empty(ops.tta_merge_workspace(B, A, D), dtype=torch.uint8, device=dev)
    ob, os_ = torch.empty((B, 100, 4), device=dev), torch.empty((B, 100), device=dev)
    oc, on = torch.empty((B, 100), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    merge = _events(lambda: ops.tta_merge(b, s, c, cnt, tf, 8, 1e-8, 0.5, 100, ws, ob, os_, oc, on), reps)
    return {"detector_postprocess_N2_D100_us_per_call": round(post, 1), "tta_merge_B1_A18_D100_us_per_call": round(merge, 1), "calls": reps}


def _host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


def end_to_end(images, tta_images, warmup):
    from aldi_amd import synthetic as syn
    from aldi_amd.predictor import Predictor
    from aldi_amd.tta import GeneralizedRCNNWithTTA
    cfg = _cfg()
    pred = Predictor(cfg)
    g = torch.Generator().manual_seed(7)
    frame = syn.make_image(1024, 2048, 12, cfg.MODEL.ROI_HEADS.NUM_CLASSES, g)[0]
    hwc = frame.permute(1, 2, 0).contiguous().cuda()
    plain = _host_ms(lambda: pred(hwc), images, warmup)
    tta = GeneralizedRCNNWithTTA(cfg, pred.model)
    small = syn.make_image(480, 640, 12, cfg.MODEL.ROI_HEADS.NUM_CLASSES, g)[0]
    small_hwc = small.permute(1, 2, 0).contiguous().cuda()
    plain_small = _host_ms(lambda: pred(small_hwc), images, warmup)
    inp = [{"image": small.cuda(), "height": 480, "width": 640}]
    n = len(tta(inp)[0]["instances"])
    t = _host_ms(lambda: tta(inp), tta_images, 1)
    return {"predictor": {"raw_size": [1024, 2048], "min_size_test": 1024, "max_size_test": 2048, "images": images,
                          "ms_per_image": round(plain, 3), "images_per_s": round(1e3 / plain, 2)},
            "tta": {"raw_size": [480, 640], "plain_predictor_ms_per_image": round(plain_small, 3), "min_sizes": list(cfg.TEST.AUG.MIN_SIZES), "max_size": cfg.TEST.AUG.MAX_SIZE, "flip": bool(cfg.TEST.AUG.FLIP), "views": 18,
                    "batch_size": 3, "images": tta_images, "ms_per_image": round(t, 2), "detections": n,
                    "ratio_to_plain_inference": round(t / plain_small, 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=30)
    ap.add_argument("--tta-images", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_predict.json"))
    a = ap.parse_args()
    res = {"tool": "bench_predict", "device": torch.cuda.get_device_name(0), "entry_points": kernel_us()}
    res.update(end_to_end(a.images, a.tta_images, a.warmup))
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

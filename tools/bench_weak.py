"""Measurement for the device weak view (aldi_amd/aug.py weak_views, csrc/geom.hip) and the AUG.DEVICE_WEAK loader stage.
Prints ONE JSON line and writes it to --out (default profiles/bench_weak.json):

* us per view and views/s of `launch_weak_views` (pinned upload of descriptors + tables, then the launches; images resident in HBM,
  parameters pre-drawn) for batches of 8, in both kernel arms (tuning knob resize_fused 1 / 0): device events around 500 back-to-back
  calls, i.e. the rate of the whole call, not a kernel time; the host's time to issue the calls is beside it:
    - 1024 x 2048 -> the eight MIN_SIZE_TRAIN sizes of the reference's Base-RCNN-FPN.yaml (800 .. 1024, MAX_SIZE_TRAIN 2048), one each,
    - 480 x 640 -> 800 x 1067;
* host Pillow `Image.resize(BILINEAR)` ms per view on the same box, where Pillow is importable;
* trainer-loop ms/step at 1333 x 800, AUG.DEVICE_WEAK + AUG.DEVICE_STRONG (raw 600 x 1000 host images, resized on the device) against
  AUG.DEVICE_STRONG alone (host weak views of 800 x 1333): same process, same trainer, alternating blocks (DESIGN.md section 9's method).

Recorded, not gated.  The bound beside the numbers: one 800 x 1333 view reads and writes about 3.2 + 3.2 MB (6 + 6 MB for a
1024 x 2048 frame), a few microseconds of HBM traffic -- far below what the strong chain's view_kernel already costs per view."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from aldi_amd import _lib as L
from aldi_amd import aug

REF_MIN_SIZE_TRAIN, REF_MAX_SIZE_TRAIN = (800, 832, 864, 896, 928, 960, 992, 1024), 2048


def cases():
    rse = aug.ResizeShortestEdge
    city = [aug.WeakParams(1024, 2048, *rse.get_output_shape(1024, 2048, s, REF_MAX_SIZE_TRAIN), flip=bool(i % 2)) for i, s in enumerate(REF_MIN_SIZE_TRAIN)]
    voc = [aug.WeakParams(480, 640, *rse.get_output_shape(480, 640, 800, 1333), flip=bool(i % 2)) for i in range(8)]
    return {"1024x2048_to_ref_min_sizes": city, "480x640_to_800x1067": voc}


def device_us(reps=500):
    out = {}
    g = np.random.default_rng(0)
    for name, params in cases().items():
        imgs = [torch.from_numpy(g.integers(0, 256, (p.h, p.w, 3), dtype=np.uint8)).cuda() for p in params]
        mb = sum(3 * (p.h * p.w + p.new_h * p.new_w) for p in params) / len(params) / 1e6
        for fused in (1, 0):
            L.set_tuning("resize_fused", fused)
            for _ in range(3):
                aug.launch_weak_views(imgs, params)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(reps):
                aug.launch_weak_views(imgs, params)
            e1.record()
            t_issue = time.perf_counter() - t0
            torch.cuda.synchronize()
            us = 1e3 * e0.elapsed_time(e1) / reps / len(params)
            out[f"{name}_{'fused' if fused else 'two_pass'}"] = {"us_per_view": round(us, 1), "views_per_s": round(1e6 / us, 1), "u8_mb_per_view": round(mb, 2),
                                                                 "gb_per_s": round(mb * 1e3 / us, 1), "host_issue_us_per_view": round(1e6 * t_issue / reps / len(params), 1)}
        L.reset_tuning()
    return out


def pillow_ms(reps=5):
    """host Pillow ms per view; also holds the device bytes to Pillow's at these sizes (both arms, flip as in the case)"""
    try:
        from PIL import Image
    except ImportError:
        return None
    out = {}
    g = np.random.default_rng(0)
    for name, params in cases().items():
        t_all = 0.0
        for i, p in enumerate(params):
            arr = g.integers(0, 256, (p.h, p.w, 3), dtype=np.uint8)
            im = Image.fromarray(arr)
            if i < 2:
                ref = np.asarray(im.resize((p.new_w, p.new_h), Image.BILINEAR))
                ref = ref[:, ::-1] if p.flip else ref
                for fused in (1, 0):
                    L.set_tuning("resize_fused", fused)
                    got = aug.weak_views([torch.from_numpy(arr).cuda()], [p], chw_out=False)[0].cpu().numpy()
                    assert np.array_equal(got, ref), (name, p, fused)
                L.reset_tuning()
            t = time.perf_counter()
            for _ in range(reps):
                np.asarray(im.resize((p.new_w, p.new_h), Image.BILINEAR))
            t_all += (time.perf_counter() - t) / reps
        out[name] = round(1e3 * t_all / len(params), 3)
    return out


class _Fixed:
    """the same records every step (fresh dict copies), like bench.py's FixedGpuLoader"""
    def __init__(self, recs):
        self.recs = recs

    def __iter__(self):
        while True:
            yield [dict(r) for r in self.recs]


def trainer_ab(steps, warmup, H=800, W=1333, raw=(600, 1000)):
    from aldi_amd import synthetic as syn
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.dataloader import DeviceStrongAugLoader, WeakStrongDataloader, device_strong_seed, device_weak_seed
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SEED", 1, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W, "SOLVER.BASE_LR", 1e-4,
                         "INPUT.MIN_SIZE_TRAIN", (H,), "INPUT.MAX_SIZE_TRAIN", W])
    weak = aug.get_weak_augs(cfg, True)
    assert weak[0].get_output_shape(raw[0], raw[1], H, W) == (H, W), "the raw size must resize to the step's input size"
    random.seed(1234)
    torch.manual_seed(100)
    tr = ALDITrainer(cfg)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    g = torch.Generator().manual_seed(100)
    full, small = [], []
    for labeled in (True, False):
        a, b = [], []
        for _ in range(2):
            for (h, w), dst in (((H, W), a), (raw, b)):
                img, inst = syn.make_image(h, w, 10, K, g)
                if not labeled:
                    inst = {"image_size": (h, w), "gt_boxes": torch.zeros(0, 4), "gt_classes": torch.zeros(0, dtype=torch.int64)}
                dst.append({"img_weak": img, "instances": inst})
        full.append(a)
        small.append(b)
    contents = tuple(cfg.DATASETS.BATCH_CONTENTS)
    loaders = {
        "strong": WeakStrongDataloader(DeviceStrongAugLoader(_Fixed(full[0]), aug.get_strong_augs(cfg, True), device_strong_seed(1, 0, True)),
                                       DeviceStrongAugLoader(_Fixed(full[1]), aug.get_strong_augs(cfg, False), device_strong_seed(1, 0, False)), contents),
        "weak_strong": WeakStrongDataloader(
            DeviceStrongAugLoader(_Fixed(small[0]), aug.get_strong_augs(cfg, True), device_strong_seed(1, 0, True), weak=weak, weak_seed=device_weak_seed(1, 0, True)),
            DeviceStrongAugLoader(_Fixed(small[1]), aug.get_strong_augs(cfg, False), device_strong_seed(1, 0, False), weak=weak, weak_seed=device_weak_seed(1, 0, False)),
            contents)}
    tr.iter = 0

    def run(loader, n):
        tr._trainer.data_loader = loader
        tr._trainer._data_loader_iter_obj = None
        for _ in range(n):
            tr.before_step()
            tr.run_step()
            tr.after_step()
            tr.iter += 1

    res = {k: [] for k in loaders}
    for _ in range(3):
        for name, loader in loaders.items():
            run(loader, warmup)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(loader, steps)
            torch.cuda.synchronize()
            res[name].append(1e3 * (time.perf_counter() - t) / steps)
    a, b = min(res["strong"]), min(res["weak_strong"])
    return {"steps_per_block": steps, "warmup_per_block": warmup, "raw_size": list(raw), "input_size": [H, W],
            "blocks_ms": {k: [round(v, 3) for v in vs] for k, vs in res.items()},
            "strong_ms_per_step": round(a, 3), "weak_strong_ms_per_step": round(b, 3), "ratio": round(b / a, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_weak.json"))
    a = ap.parse_args()
    res = {"tool": "bench_weak", "device": torch.cuda.get_device_name(0), "batch": 8, "device_per_view": device_us(), "host_pillow_ms_per_view": pillow_ms()}
    res["device_bytes_equal_pillow_at_these_sizes"] = res["host_pillow_ms_per_view"] is not None
    if not a.no_trainer:
        res["trainer_loop_1333x800"] = trainer_ab(a.steps, a.warmup)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

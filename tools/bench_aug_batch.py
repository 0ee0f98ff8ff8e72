"""Measurement for the batched strong augmentation (aldi_amd/aug.py strong_views, csrc/aug.hip batch kernels) and the
AUG.DEVICE_STRONG loader stage.  Prints ONE JSON line (and writes it to --out):

* views/s of strong_views (draws + launches, weak views resident in HBM) at N in {1, 4, 8} for 1333x800 and 2048x1024, the
  reference chain (build_strong_augmentation + MIC) with its own random gates;
* device ms per batch of the three launches with every gate on at sigma = 2 (parameters pre-drawn, device events);
* host ms per view of draw_strong_params (the loader's draw thread does this);
* trainer-loop ms/step, AUG.DEVICE_STRONG on vs off, same process, same trainer (interleaved A/B blocks, >= 50 timed steps each).

`--trace` runs only a short fixed workload for a separate `rocprofv3 --kernel-trace --stats` run (kernel times, launch count)."""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aldi_amd import aug

SIZES = [(800, 1333), (1024, 2048)]


def chain():
    return aug.build_strong_augmentation(include_erasing=True) + [aug.RandomApply(aug.MICTransform(0.5, 32), prob=1.0)]


def weak(H, W, n, seed=0):
    g = np.random.default_rng(seed)
    return [torch.from_numpy(g.integers(0, 256, (3, H, W), dtype=np.uint8)).cuda() for _ in range(n)]


def all_on_params(H, W, rs):
    """every gate on, sigma 2 (radius 8), three erase rects of the chain's mean areas, MIC 32"""
    rects = [(10, 20, int(H * 0.35), int(W * 0.36)), (H // 2, W // 3, int(H * 0.3), int(W * 0.35)), (H // 4, W // 2, int(H * 0.3), int(W * 0.33))]
    erases = []
    for r in rects:
        sn, sp = aug.np_mt_advance(rs, 2 * r[2] * r[3] * 3)
        erases.append((r, sn, sp))
    return aug.StrongParams(H, W, colour=(1.2, 0.8, 1.1), gray=0.0, sigma=2.0, erases=erases, mic=rs.rand(round(H / 32), round(W / 32)) > 0.5)


def fp64_ops(H, W, R=8):
    """double-precision ops of the fused blur at radius R: per element and axis 1 mul + R (add, mul, add); the row axis also runs
    on the 2R halo columns of each 64-wide tile; the colour chain ~10 ops per element over the 16+2R x 64+2R loaded pixels"""
    per_axis = 1 + 3 * R
    n = H * W * 3
    return n * per_axis * ((64 + 2 * R) / 64 + 2) + n * 10 * ((16 + 2 * R) * (64 + 2 * R)) / (16 * 64)


def views_per_s(reps=30):
    out = {}
    augs = chain()
    for H, W in SIZES:
        for N in (1, 4, 8):
            vs = weak(H, W, N)
            rs, pr = np.random.RandomState(0), random.Random(0)
            for _ in range(3):
                aug.strong_views(vs, augs, np_rng=rs, py_rng=pr)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                aug.strong_views(vs, augs, np_rng=rs, py_rng=pr)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            out[f"{W}x{H}_N{N}"] = round(reps * N / dt, 1)
    return out


def device_ms(reps=50):
    out = {}
    for H, W in SIZES:
        for N in (1, 8):
            rs = np.random.RandomState(1)
            vs = weak(H, W, N)
            ps = [all_on_params(H, W, rs) for _ in range(N)]
            for _ in range(3):
                aug.launch_strong_views(vs, ps)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                aug.launch_strong_views(vs, ps)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / reps
            out[f"{W}x{H}_N{N}"] = {"ms_per_batch": round(ms, 4), "us_per_view": round(1e3 * ms / N, 1),
                                    "fp64_gops_per_view": round(fp64_ops(H, W) / 1e9, 3),
                                    "u8_mb_per_view": round(2 * 3 * H * W / 1e6, 2)}
    return out


def host_ms_per_view(n=200):
    augs = chain()
    rs, pr = np.random.RandomState(2), random.Random(2)
    out = {}
    for H, W in SIZES:
        t = time.perf_counter()
        for _ in range(n):
            aug.draw_strong_params(augs, H, W, np_rng=rs, py_rng=pr)
        out[f"{W}x{H}"] = round(1e3 * (time.perf_counter() - t) / n, 4)
        # the fills the reference draws with np.random.rand, for the same chain, on this host
        rs2, pr2 = np.random.RandomState(2), random.Random(2)
        t = time.perf_counter()
        for _ in range(min(n, 50)):
            p = aug.draw_strong_params(augs, H, W, np_rng=rs2, py_rng=pr2)
            for rect, _, _ in p.erases:
                np.random.rand(rect[2], rect[3], 3)
        out[f"{W}x{H}_with_host_rand_fills"] = round(1e3 * (time.perf_counter() - t) / min(n, 50), 4)
    return out


class _Fixed:
    """the same records every step (fresh dict copies), like bench.py's FixedGpuLoader"""
    def __init__(self, recs):
        self.recs = recs

    def __iter__(self):
        while True:
            yield [dict(r) for r in self.recs]


def trainer_ab(steps, warmup, H, W, host_weak):
    from aldi_amd import synthetic as syn
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.dataloader import DeviceStrongAugLoader, WeakStrongDataloader, device_strong_seed
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SEED", 1, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W, "SOLVER.BASE_LR", 1e-4])
    random.seed(1234)
    torch.manual_seed(100)
    tr = ALDITrainer(cfg)
    K = cfg.MODEL.ROI_HEADS.NUM_CLASSES
    g = torch.Generator().manual_seed(100)
    parts = []
    for labeled in (True, False):
        recs = []
        for _ in range(2):
            img, inst = syn.make_image(H, W, 10, K, g)
            if not labeled:
                inst = {"image_size": (H, W), "gt_boxes": torch.zeros(0, 4), "gt_classes": torch.zeros(0, dtype=torch.int64)}
            recs.append({"image": syn.strong_view(img, g).cuda(), "img_weak": img if host_weak else img.cuda(), "instances": inst})
        parts.append(recs)
    contents = tuple(cfg.DATASETS.BATCH_CONTENTS)
    off = WeakStrongDataloader(_Fixed([dict(r, img_weak=r["img_weak"].cuda()) for r in parts[0]]),
                               _Fixed([dict(r, img_weak=r["img_weak"].cuda()) for r in parts[1]]), contents)
    on = WeakStrongDataloader(DeviceStrongAugLoader(_Fixed(parts[0]), aug.get_strong_augs(cfg, True), device_strong_seed(1, 0, True)),
                              DeviceStrongAugLoader(_Fixed(parts[1]), aug.get_strong_augs(cfg, False), device_strong_seed(1, 0, False)), contents)
    tr.iter = 0

    def run(loader, n):
        tr._trainer.data_loader = loader
        tr._trainer._data_loader_iter_obj = None
        for _ in range(n):
            tr.before_step()
            tr.run_step()
            tr.after_step()
            tr.iter += 1

    res = {"off": [], "on": []}
    for blk in range(2):
        for name, loader in (("off", off), ("on", on)):
            run(loader, warmup)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(loader, steps)
            torch.cuda.synchronize()
            res[name].append(1e3 * (time.perf_counter() - t) / steps)
    off_ms, on_ms = min(res["off"]), min(res["on"])
    return {"steps_per_block": steps, "warmup_per_block": warmup, "blocks_ms": {k: [round(v, 3) for v in vs] for k, vs in res.items()},
            "off_ms_per_step": round(off_ms, 3), "on_ms_per_step": round(on_ms, 3), "ratio_on_off": round(on_ms / off_ms, 4),
            "weak_views": "host (pinned async copy)" if host_weak else "device"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:                                         # 5 batches of 8 all-gates-on views + 5 chain batches, for the kernel trace
        rs = np.random.RandomState(3)
        vs = weak(800, 1333, 8)
        ps = [all_on_params(800, 1333, rs) for _ in range(8)]
        for _ in range(5):
            aug.launch_strong_views(vs, ps)
        for _ in range(5):
            aug.strong_views(vs, chain(), np_rng=rs, py_rng=random.Random(3))
        torch.cuda.synchronize()
        print(json.dumps({"trace": "5 x (8 views all gates on, 1333x800) + 5 x (8 views, chain draws)"}))
        return
    res = {"tool": "bench_aug_batch", "device": torch.cuda.get_device_name(0), "views_per_s": views_per_s(), "device_all_gates_on": device_ms(),
           "host_draw_ms_per_view": host_ms_per_view(),
           "trainer_loop_1333x800": [trainer_ab(a.steps, a.warmup, 800, 1333, False), trainer_ab(a.steps, a.warmup, 800, 1333, True)]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

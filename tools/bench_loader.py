#!/usr/bin/env python
"""File-backed loader measurement -> profiles/bench_loader.json.  Recorded, not gated: the decode rate is a
property of the host.

Writes its own dataset -- 1024 x 2048 random-content images as binary PPM, and as PNG where Pillow is installed -- into a temporary
directory, then reports
  * records/s of FileDetectionLoader alone (mapper included, no device) at 1, 4 and 16 decode threads, per file format;
  * trainer ms/step with DATASETS.FILES (PPM; 2 + 2 raw 1024 x 2048 images per step, resized on the device to 667 x 1333) against the
    synthetic DEVICE_WEAK + DEVICE_STRONG loader with raw images of the same size, in alternating blocks in one process, best block per
    arm (the method of tools/bench_weak.py)."""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, NIMG = 1024, 2048, 16


def write_dataset(root, fmt):
    """NIMG images + a COCO json -> the json's path"""
    images, annos = [], []
    for i in range(NIMG):
        img = np.random.RandomState(900 + i).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        fn = f"{fmt}_{i:03d}.{fmt}"
        if fmt == "ppm":
            with open(os.path.join(root, fn), "wb") as f:
                f.write(b"P6\n%d %d\n255\n" % (W, H) + img.tobytes())
        else:
            from PIL import Image
            Image.fromarray(img).save(os.path.join(root, fn))
        images.append(dict(id=i + 1, file_name=fn, height=H, width=W))
        for k in range(8):
            x, y = 100 + 200 * k, 80 + 90 * k
            annos.append(dict(id=len(annos) + 1, image_id=i + 1, category_id=1 + k % 8, bbox=[x, y, 160, 120], iscrowd=0, area=160 * 120))
    path = os.path.join(root, f"{fmt}.json")
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=annos, categories=[dict(id=c, name=f"c{c}") for c in range(1, 9)]), f)
    return path


def base_cfg(*pairs):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SEED", 1, "SOLVER.BASE_LR", 1e-4, "AUG.DEVICE_WEAK", True, "AUG.DEVICE_STRONG", True,
                         "INPUT.MIN_SIZE_TRAIN", (800,), "INPUT.MAX_SIZE_TRAIN", 1333, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W] + list(pairs))
    return cfg


def loader_rate(name, threads, batches=12, bs=4):
    from aldi_amd.dataloader import FileDetectionLoader, TrainingSampler
    from aldi_amd.datasets import get_detection_dataset_dicts
    from aldi_amd.mapper import DatasetMapper
    dicts = get_detection_dataset_dicts([name])
    ld = FileDetectionLoader(dicts, DatasetMapper(base_cfg(), True, True), bs, TrainingSampler(len(dicts), True, 1), num_threads=threads)
    it = iter(ld)
    next(it)                                                           # (threads started, files in the page cache)
    t = time.perf_counter()
    for _ in range(batches):
        next(it)
    dt = time.perf_counter() - t
    ld.close()
    return round(batches * bs / dt, 1)


def trainer_ab(name, steps, warmup, threads):
    import torch
    from aldi_amd.trainer import ALDITrainer
    random.seed(1234)
    torch.manual_seed(100)
    cfg = base_cfg()
    tr = ALDITrainer(cfg)
    files_cfg = base_cfg("DATASETS.FILES", True, "DATASETS.TRAIN", (name,), "DATASETS.UNLABELED", (name,), "DATALOADER.NUM_WORKERS", threads)
    loaders = {"synthetic": ALDITrainer.build_train_loader(cfg), "files": ALDITrainer.build_train_loader(files_cfg)}
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
        for key, loader in loaders.items():
            run(loader, warmup)
            torch.cuda.synchronize()
            t = time.perf_counter()
            run(loader, steps)
            torch.cuda.synchronize()
            res[key].append(1e3 * (time.perf_counter() - t) / steps)
    a, b = min(res["synthetic"]), min(res["files"])
    return {"steps_per_block": steps, "warmup_per_block": warmup, "decode_threads": threads, "file_format": "ppm", "images_per_step": 4,
            "blocks_ms": {k: [round(v, 3) for v in vs] for k, vs in res.items()},
            "synthetic_ms_per_step": round(a, 3), "files_ms_per_step": round(b, 3), "ratio": round(b / a, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--threads", type=int, default=4, help="decode threads of the trainer comparison (DATALOADER.NUM_WORKERS)")
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_loader.json"))
    a = ap.parse_args()
    from aldi_amd import datasets
    try:
        import PIL  # noqa: F401
        formats = ["ppm", "png"]
    except ImportError:
        formats = ["ppm"]
    root = tempfile.mkdtemp(prefix="bench_loader_")
    try:
        res = {"tool": "bench_loader", "image_size": [H, W], "images": NIMG, "formats": formats, "usable_cpus": len(os.sched_getaffinity(0)),
               "records_per_s": {}}
        for fmt in formats:
            datasets.register_coco_instances(f"bench_loader_{fmt}", {}, write_dataset(root, fmt), root)
            res["records_per_s"][fmt] = {str(t): loader_rate(f"bench_loader_{fmt}", t) for t in (1, 4, 16)}
        if not a.no_trainer:
            import torch
            res["device"] = torch.cuda.get_device_name(0)
            res["trainer_loop"] = trainer_ab("bench_loader_ppm", a.steps, a.warmup, a.threads)
            ms = res["trainer_loop"]["files_ms_per_step"]
            res["records_per_s_the_step_needs"] = round(4 * 1e3 / ms, 1)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

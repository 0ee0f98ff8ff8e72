"""Measurement for the device COCO evaluator (aldi_amd/evaluation.py DeviceCOCOEvaluator, csrc/eval.hip, TEST.DEVICE_EVAL).
Prints ONE JSON line (and writes it to --out).  In one process, on the 500-image form of synthetic.make_eval_scene (2048 x 1024,
8 categories, 100 detections per image, device-resident Instances, one image per `process` call):

* host path: `Detectron2COCOEvaluatorAdapter.process` over all images + `evaluate()` (the yardstick);
* device path: `DeviceCOCOEvaluator.process` over the same Instances + `evaluate()` including the final copy;
  both with a device synchronise at either end, median of --repeats runs after a warm-up; and whether the two result dicts are equal;
* device time of the stages of one evaluation (segment sorts, match, category sorts, accumulate; device events);
* with --detail: both evaluators with `detail=True` and `score_thresh=--score-thresh` (TEST.EVAL_DETAIL: AR, per-category AP,
  precision / recall above the cut), `equal` over all keys, and the stage times with the detail counters on
  (`device_stage_ms`) and off (`device_stage_ms_detail_off`) on the same detections: medians of 5 evaluations each, alternating;
* with --trainer: wall time of one `ALDITrainer.test()` on the default synthetic validation split (N = SYNTHETIC.VAL_IMAGES = 8
  images) with TEST.DEVICE_EVAL off and on, same weights -- stated for those 8 images, not extrapolated."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aldi_amd import synthetic as syn
from aldi_amd.evaluation import DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
from aldi_amd.structures import Boxes, Instances


def scene(num_images, num_classes):
    records, dets = syn.make_eval_scene(num_images, num_classes, 1024, 2048, seed=0)
    feed = []
    for r, d in zip(records, dets):
        inst = Instances((r["height"], r["width"]))
        inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(d["boxes"].cuda()), d["scores"].cuda(), d["classes"].cuda()
        feed.append(([dict(image_id=r["image_id"], height=r["height"], width=r["width"])], [inst]))
    return records, feed


def timed(ev, feed, repeats, warmup=1):
    ts, res = [], None
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.reset()
        for inputs, outputs in feed:
            ev.process(inputs, outputs)
        res = ev.evaluate()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts, res


def same(a, b):
    return list(a) == list(b) and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def stages(dev, feed, detail=None):
    dev.reset()
    for inputs, outputs in feed:
        dev.process(inputs, outputs)
    marks = []

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((name, e))
    mark("start")
    arrays = dev._compact()
    mark("postprocess")
    dev._evaluate_device(arrays, mark, detail=detail).cpu()
    torch.cuda.synchronize()
    return {n: round(marks[i][1].elapsed_time(e), 4) for i, (n, e) in enumerate(marks[1:])}


def stages_on_off(dev, feed, repeats=5):
    """-> (detail on, detail off): per-stage medians of `repeats` evaluations each, alternating, after one warm-up of both"""
    runs = {False: [], True: []}
    for k in range(repeats + 1):
        for detail in (False, True):
            r = stages(dev, feed, detail)
            if k:
                runs[detail].append(r)
    med = lambda rs: {n: round(statistics.median(r[n] for r in rs), 4) for n in rs[0]}
    return med(runs[True]), med(runs[False])


def trainer_test(repeats=3):
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.trainer import ALDITrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(root, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.AMP.ENABLED", True, "SEED", 1])
    random.seed(0)
    torch.manual_seed(1)
    tr = ALDITrainer(cfg)
    out = {"images": int(cfg.get("SYNTHETIC", {}).get("VAL_IMAGES", 8))}
    res = {}
    for on in (False, True, False, True):
        cfg.merge_from_list(["TEST.DEVICE_EVAL", on])
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[on] = ALDITrainer.test(cfg, tr.ema.model)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out.setdefault("device_eval_on_ms" if on else "device_eval_off_ms", []).extend(round(t * 1e3, 2) for t in ts)
    out["equal"] = same(res[False]["bbox"], res[True]["bbox"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--detail", action="store_true")
    ap.add_argument("--score-thresh", type=float, default=0.8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    records, feed = scene(a.images, a.classes)
    kw = dict(detail=True, score_thresh=a.score_thresh) if a.detail else {}
    host = Detectron2COCOEvaluatorAdapter("val", records, a.classes, distributed=False, **kw)
    dev = DeviceCOCOEvaluator("val", records, a.classes, distributed=False, **kw)
    d_med, d_all, d_res = timed(dev, feed, max(5, a.repeats))
    h_med, h_all, h_res = timed(host, feed, max(5, a.repeats))
    out = {"bench": "eval_device", "gpu": torch.cuda.get_device_name(0), "images": a.images, "classes": a.classes,
           "ground_truth": sum(len(r["annotations"]) for r in records), "detections": sum(len(o[0]) for _, o in feed),
           "host_ms": round(h_med * 1e3, 2), "device_ms": round(d_med * 1e3, 2), "host_over_device": round(h_med / d_med, 1),
           "host_runs_ms": [round(t * 1e3, 1) for t in h_all], "device_runs_ms": [round(t * 1e3, 2) for t in d_all],
           "equal": same(h_res["bbox"], d_res["bbox"]), "bbox": dict(d_res["bbox"])}
    if a.detail:
        out["detail"], out["keys"] = True, len(d_res["bbox"])
        out["device_stage_ms"], out["device_stage_ms_detail_off"] = stages_on_off(dev, feed)
    else:
        out["device_stage_ms"] = stages(dev, feed)
    if a.trainer:
        out["trainer_test"] = trainer_test()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

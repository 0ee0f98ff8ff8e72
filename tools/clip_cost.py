#!/usr/bin/env python3
"""Device time of the optimizer step of the flat R50-FPN state with SOLVER.CLIP_GRADIENTS off / value / norm / full_model.

usage: clip_cost.py [--num-classes 80] [--steps 20] [--warmup 5] [--fp32]
Times Weights.sgd_step (what EngineSGD.step launches) with device events over `steps` steps after `warmup`, on a random gradient,
and the norm pass alone.  Prints ONE JSON line: microseconds per step, the ratio to clipping off, and the ratio the bytes predict
(the norm types read the gradient once more: 4 bytes on top of the pass's 20 + 2 per element)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-classes", type=int, default=80)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fp32", action="store_true", help="no bf16 compute copy")
    a = ap.parse_args()
    from aldi_amd import ops
    from aldi_amd.arch import ParamLayout
    from aldi_amd.engine import Weights
    lay = ParamLayout(a.num_classes)
    dtype = torch.float32 if a.fp32 else torch.bfloat16
    wts = Weights(lay, torch.device("cuda"), dtype, trainable=True)
    wts.master.normal_(0, 0.02)
    wts.grad.normal_(0, 1e-3)
    wts.mom.zero_()
    plan = wts.clip_plan()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
        ev[0].record()
        for i in range(a.steps):
            fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ts = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(a.steps))
        return {"median_us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}
    bytes_per = 20 + (0 if a.fp32 else 2)
    specs = {"off": None, "value": ops.ClipSpec("value", 1e-3, 2.0), "norm": ops.ClipSpec("norm", 0.02, 2.0), "full_model": ops.ClipSpec("full_model", 1.0, 2.0)}
    out = {"n_train": lay.n_train, "n_segments": plan.n_segs, "n_chunks": plan.n_chunks, "dtype": str(dtype).replace("torch.", ""), "steps": a.steps}
    for name, spec in specs.items():
        out[name] = timed(lambda: wts.sgd_step(1e-4, 0.9, 1e-4, clip=spec))
    out["norm_pass_alone"] = timed(lambda: ops.grad_seg_norms(wts.grad, plan, 2.0))
    for name in ("value", "norm", "full_model"):
        out[name]["ratio_to_off"] = round(out[name]["median_us"] / out["off"]["median_us"], 3)
        out[name]["ratio_by_bytes"] = round(1.0 if name == "value" else (bytes_per + 4) / bytes_per, 3)
    out["off"]["tb_per_s"] = round(lay.n_train * bytes_per / out["off"]["median_us"] / 1e6, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

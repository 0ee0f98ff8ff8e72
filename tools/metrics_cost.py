#!/usr/bin/env python3
"""What SOLVER.LOG_PERIOD costs per step on the benchmark shape (bench.make_cfg(1, 800, 1333, ...): 2 + 2 images, bf16, fused step + graphs).

usage: metrics_cost.py [--block 40] [--rounds 4] [--warmup 24] [--period 20] [--out FILE]
ONE process builds its trainers on the same fixed batch: A (LOG_PERIOD 0), A' (LOG_PERIOD 0 again) and B (LOG_PERIOD `period`), warms
each up (graph capture and B's first flush included), then times alternating blocks of `block` steps for `rounds` rounds -- A, A', B, C, A,
... -- each block ending in a synchronise.  The yardstick is the A-vs-A' difference of the same run: two trainers that launch the same work.
C records every step like B but its window (4096) is longer than the run, so it never flushes: C - A is the per-step part (the record
launch and the statistics launches), B - C the flushes.  Prints ONE JSON line: per trainer the ms/step of every block, their median,
minimum and maximum; B's flush count and host times (this tool wraps B's `record` and `flush`; the wait of a flush is timed as a
synchronise in front of it); B - A, C - A and A' - A of the medians.
Four full-size trainers (student, teacher and step graphs each) live in this process at once: about four times the benchmark's memory."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--period", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import bench
    from aldi_amd import synthetic as syn
    from aldi_amd.trainer import ALDITrainer
    dev = torch.device("cuda", torch.cuda.current_device())
    out_dir = tempfile.mkdtemp(prefix="metrics_cost_")

    def build(period):
        cfg = bench.make_cfg(1, 800, 1333, False)
        cfg.merge_from_list(["SOLVER.LOG_PERIOD", period, "OUTPUT_DIR", os.path.join(out_dir, "p%d" % period), "SOLVER.CHECKPOINT_PERIOD", 0,
                             "SOLVER.MAX_ITER", 10 ** 6])
        random.seed(1234)
        torch.manual_seed(100)
        tr = ALDITrainer(cfg)
        data = syn.make_batch(2, 2, 800, 1333, cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=100)
        tr._trainer.data_loader = bench.FixedGpuLoader(data, dev)
        tr._trainer._data_loader_iter_obj = None
        tr.iter = 0
        return tr

    def steps(tr, n):
        for _ in range(n):
            tr.before_step()
            tr.run_step()
            tr.after_step()
            tr.iter += 1

    trainers = [("A", build(0)), ("A2", build(0)), ("B", build(a.period)), ("C", build(4096))]
    assert a.warmup + a.block * a.rounds < 4096
    rec = trainers[2][1].metric_recorder
    host = {"record": 0.0, "records": 0, "flushes": []}       # host seconds inside B's record(); (waiting, rest) per flush that had rows
    rec_record, rec_flush = rec.record, rec.flush

    def timed_record(*args, **kw):
        t0 = time.perf_counter()
        rec_record(*args, **kw)
        host["record"] += time.perf_counter() - t0
        host["records"] += 1

    def timed_flush():
        if not rec.pending():
            return rec_flush()
        t0 = time.perf_counter()
        torch.cuda.synchronize()                     # what the flush would wait for
        t1 = time.perf_counter()
        out_ = rec_flush()
        host["flushes"].append((t1 - t0, time.perf_counter() - t1))
        return out_
    rec.record, rec.flush = timed_record, timed_flush
    n_flush_c = [0]
    rec_c = trainers[3][1].metric_recorder
    c_flush = rec_c.flush
    rec_c.flush = lambda: (n_flush_c.__setitem__(0, n_flush_c[0] + bool(rec_c.pending())), c_flush())[1]
    for _, tr in trainers:
        steps(tr, a.warmup)
        torch.cuda.synchronize()
    ms = {name: [] for name, _ in trainers}
    for _ in range(a.rounds):
        for name, tr in trainers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(tr, a.block)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / a.block * 1e3)
    out = {"shape": "r50_fpn 2+2 800x1333 bf16 fused+graphs", "block": a.block, "rounds": a.rounds, "log_period": a.period}
    for name, _ in trainers:
        v = ms[name]
        out[name] = {"ms_per_step_blocks": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    fs = trainers[2][1]._trainer._fused_step
    out["B"]["flushes"] = len(host["flushes"])
    out["B"]["host_us_per_step_in_record"] = round(host["record"] / max(host["records"], 1) * 1e6, 1)
    out["B"]["host_ms_per_flush_waiting"] = round(statistics.median(w for w, _ in host["flushes"]) * 1e3, 3)
    out["B"]["host_ms_per_flush_after_wait"] = round(statistics.median(t for _, t in host["flushes"]) * 1e3, 3)
    out["C"]["flushes"] = n_flush_c[0]
    out["C_minus_A_ms"] = round(out["C"]["median"] - out["A"]["median"], 4)
    out["B"]["graph_replays_b"] = fs.stats.get("replays_b")
    out["A2_minus_A_ms"] = round(out["A2"]["median"] - out["A"]["median"], 4)
    out["B_minus_A_ms"] = round(out["B"]["median"] - out["A"]["median"], 4)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

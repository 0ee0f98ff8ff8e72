"""Training metrics: detectron2's EventStorage / JSONWriter / CommonMetricPrinter surface fed from a DEVICE ring.

The reference logs with one `.item()` per loss per step (SimpleTrainer._write_metrics -> EventStorage -> writers): a host wait every
iteration.  Here the step's loss scalars and the head counters are copied into a device ring by ONE small launch per iteration
(`aldi_metrics_record`, csrc/trainstats.hip) and reach the host once per logging window (`DeviceMetricRecorder.flush`): one
device->host copy, the only place where the host may wait.  `SOLVER.LOG_PERIOD` (0 = off: none of this exists) is the window.

Window statistics (`window_stats`) are computed on the host in double from the copied fp32 values: per row `total_loss` = the sum of
the row's loss values in key order; per key (and for total_loss, data_time, time) numpy's median over the window's rows; `lr` the latest
value; `eta_seconds` = median time x remaining iterations; head statistics are per-row ratios of the counts of detectron2's
`_log_classification_stats` / the sampled RPN labels, then the median over the rows whose denominator is not 0 (no such row: no key).

Deliberate deviation: detectron2 writes ONE unsuffixed head-statistics key that the last micro-step of the iteration overwrites.  A
mix of source and pseudo-labelled passes is of no use, so the head keys carry the micro-step suffix the loss keys carry
(`fast_rcnn/cls_accuracy_source_strong`, `rpn/num_pos_anchors_distill`, ...).

detectron2 is not installed where this project is tested: this module restates its writers (detectron2/utils/events.py) and its smoothing
(median over the window) from their documented behaviour and is not pinned to them by a test.
"""
from __future__ import annotations

import datetime
import json
import logging
import os
from collections import OrderedDict, defaultdict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.distributed as dist

BOX_STAT_NAMES = ("num_instances", "num_accurate", "num_fg", "fg_num_accurate", "num_false_negative")
RPN_STAT_NAMES = ("num_pos_anchors", "num_neg_anchors")
STAT_NAMES = BOX_STAT_NAMES + RPN_STAT_NAMES
MAX_FLOATS, MAX_INTS = 64, 32                      # ALDI_METRICS_MAX_FLOATS / ALDI_METRICS_MAX_INTS (include/aldi_hip.h)

# ------------------------------------------------------------------------------------------------ storage
_CURRENT_STORAGE_STACK: List["EventStorage"] = []


def get_event_storage() -> "EventStorage":
    """the EventStorage of the innermost `with EventStorage(...)` block (detectron2.utils.events.get_event_storage)"""
    assert len(_CURRENT_STORAGE_STACK), "get_event_storage() has to be called inside a 'with EventStorage(...)' context!"
    return _CURRENT_STORAGE_STACK[-1]


class EventStorage:
    """the minimal detectron2 surface: scalars with their iteration, the latest value of each, the history of one name"""
    def __init__(self, start_iter: int = 0):
        self._history: Dict[str, List[Tuple[float, int]]] = defaultdict(list)
        self._latest: Dict[str, Tuple[float, int]] = {}
        self._iter = int(start_iter)

    @property
    def iter(self) -> int:
        return self._iter

    @iter.setter
    def iter(self, value: int):
        self._iter = int(value)

    def step(self):
        self._iter += 1

    def put_scalar(self, name: str, value, cur_iter: Optional[int] = None):
        it = self._iter if cur_iter is None else int(cur_iter)
        value = float(value)
        self._history[name].append((value, it))
        self._latest[name] = (value, it)

    def put_scalars(self, *, cur_iter: Optional[int] = None, **kwargs):
        for k, v in kwargs.items():
            self.put_scalar(k, v, cur_iter=cur_iter)

    def latest(self) -> Dict[str, Tuple[float, int]]:
        return self._latest

    def history(self, name: str) -> List[Tuple[float, int]]:
        if name not in self._history:
            raise KeyError("No history metric available for {}!".format(name))
        return self._history[name]

    def __enter__(self):
        _CURRENT_STORAGE_STACK.append(self)
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        assert _CURRENT_STORAGE_STACK[-1] is self
        _CURRENT_STORAGE_STACK.pop()


# ------------------------------------------------------------------------------------------------ window statistics
def head_stat_keys(suffix: str) -> Dict[str, Tuple[str, str]]:
    """head-statistics key -> (numerator, denominator) among STAT_NAMES + "images" + "num_bg" for one micro-step suffix"""
    s = "_" + suffix
    return OrderedDict([
        ("fast_rcnn/cls_accuracy" + s, ("num_accurate", "num_instances")),
        ("fast_rcnn/fg_cls_accuracy" + s, ("fg_num_accurate", "num_fg")),
        ("fast_rcnn/false_negative" + s, ("num_false_negative", "num_fg")),
        ("roi_head/num_fg_samples" + s, ("num_fg", "images")),
        ("roi_head/num_bg_samples" + s, ("num_bg", "images")),
        ("rpn/num_pos_anchors" + s, ("num_pos_anchors", "images")),
        ("rpn/num_neg_anchors" + s, ("num_neg_anchors", "images")),
    ])


def window_stats(keys: Sequence[str], values, *, data_time=None, time=None, lr=None, iteration: int = 0, max_iter: Optional[int] = None,
                 suffixes: Sequence[str] = (), counts=None, images=None) -> "OrderedDict[str, float]":
    """one logging window -> the scalars of its flush.  values [rows][len(keys)] (the copied fp32 loss values), data_time / time [rows]
    host seconds, counts [rows][7 * len(suffixes)] (STAT_NAMES per suffix), images [rows][len(suffixes)] the micro-step's image count.
    Everything in double; medians are numpy's."""
    out: "OrderedDict[str, float]" = OrderedDict()
    v = np.asarray(values, dtype=np.float64).reshape(-1, len(keys))
    rows = v.shape[0]
    if rows == 0:
        return out
    total = np.zeros(rows, dtype=np.float64)
    for j in range(len(keys)):                     # (key order: the sum a reader of the row would form)
        total = total + v[:, j]
    out["total_loss"] = float(np.median(total))
    for j, k in enumerate(keys):
        out[k] = float(np.median(v[:, j]))
    if data_time is not None and len(data_time):
        out["data_time"] = float(np.median(np.asarray(data_time, dtype=np.float64)))
    if time is not None and len(time):
        out["time"] = float(np.median(np.asarray(time, dtype=np.float64)))
        if max_iter is not None:
            out["eta_seconds"] = out["time"] * max(int(max_iter) - int(iteration) - 1, 0)
    if lr is not None:
        out["lr"] = float(lr)
    if len(suffixes):
        cnt = np.asarray(counts, dtype=np.float64).reshape(rows, len(suffixes), len(STAT_NAMES))
        img = np.asarray(images, dtype=np.float64).reshape(rows, len(suffixes))
        for si, suffix in enumerate(suffixes):
            col = {n: cnt[:, si, j] for j, n in enumerate(STAT_NAMES)}
            col["images"] = img[:, si]
            col["num_bg"] = col["num_instances"] - col["num_fg"]
            for key, (num, den) in head_stat_keys(suffix).items():
                ok = col[den] != 0
                if ok.any():
                    out[key] = float(np.median(col[num][ok] / col[den][ok]))
    return out


def reduce_window(sums: torch.Tensor, n_mean: int, maxes: torch.Tensor, world: Optional[int] = None):
    """the data-parallel reduction of one window, in place, on whatever device the tensors live on: `sums` [rows][n_mean + n_counts]
    (double) is ONE all_reduce(SUM) -- its first n_mean columns (the losses) are then divided by the world size = the mean over ranks, the
    others (the counts, the image counts) stay sums -- and `maxes` (data_time, time: per-rank host measurements) one all_reduce(MAX)"""
    world = dist.get_world_size() if world is None else world
    dist.all_reduce(sums, op=dist.ReduceOp.SUM)
    sums[:, :n_mean] /= world
    dist.all_reduce(maxes, op=dist.ReduceOp.MAX)
    return sums, maxes


# ------------------------------------------------------------------------------------------------ device side
class HeadStatSink:
    """where the R-CNN engine's statistics launches add their counts: seven int32 device words (STAT_NAMES) per micro-step suffix, in one
    persistent buffer (captured graphs keep its addresses).  `aldi_metrics_record` copies the words into the ring and clears them, so every
    iteration starts from 0 without a fill launch.  The launches are the engine's (engine.py: beside its loss kernels, same stream, same
    inputs); the image count per suffix is host knowledge of the step's driver (`set_images`)."""
    MAX_SUFFIXES = MAX_INTS // len(STAT_NAMES)

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = torch.zeros(MAX_INTS, dtype=torch.int32, device=self.device)
        self.suffixes: List[str] = []
        self.images: Dict[str, int] = {}
        self.current: Optional[str] = None           # the sequential driver's micro-step (the fused step names its chunks itself)

    def words(self, suffix: str) -> torch.Tensor:
        if suffix not in self.suffixes:
            if len(self.suffixes) >= self.MAX_SUFFIXES:
                raise ValueError(f"head statistics: more than {self.MAX_SUFFIXES} micro-step suffixes ({self.suffixes + [suffix]})")
            self.suffixes.append(suffix)
        i = self.suffixes.index(suffix) * len(STAT_NAMES)
        return self.buf[i: i + len(STAT_NAMES)]

    def set_images(self, images: Dict[str, int]):
        """this iteration's image count per suffix (replaces the previous iteration's)"""
        self.images = dict(images)
        for s in images:
            self.words(s)

    def add_images(self, suffix: str, n: int):
        self.words(suffix)
        self.images[suffix] = self.images.get(suffix, 0) + int(n)

    def box(self, pred: torch.Tensor, K: int, cls: torch.Tensor, ranges: Sequence[Tuple[str, int, int]]):
        """aldi_box_cls_stats for (suffix, r0, r1) row ranges of the box predictor's rows"""
        from . import ops
        merged: List[list] = []                      # adjacent ranges of one suffix (the chunks of one micro-step) become one range
        for s, r0, r1 in ranges:
            if r1 <= r0:
                continue
            if merged and merged[-1][0] == s and merged[-1][2] == r0:
                merged[-1][2] = r1
            else:
                merged.append([s, r0, r1])
        for i in range(0, len(merged), ops.STATS_MAX_RANGES):          # (a launch takes ALDI_STATS_MAX_RANGES ranges)
            ops.box_cls_stats(pred, K, cls, [(r0, r1, self.words(s)[:5]) for s, r0, r1 in merged[i: i + ops.STATS_MAX_RANGES]])

    def rpn(self, suffix: str, labels: torch.Tensor):
        """aldi_rpn_label_counts of one micro-step's sampled labels [N][sum A]"""
        from . import ops
        if labels.numel():
            ops.rpn_label_counts(labels, self.words(suffix)[5:7])

    def counter_tensors(self) -> List[torch.Tensor]:
        n = len(self.suffixes) * len(STAT_NAMES)
        return [self.buf[j: j + 1] for j in range(n)]


class DeviceMetricRecorder:
    """owns the device ring (`period` rows), its pinned host mirror and the `first_bad_iter` word.  `record` is one launch on the current
    stream; `flush` is one device->host copy (after one all_reduce of the window under data parallelism) and returns the window's
    statistics, or raises FloatingPointError when a recorded loss was not finite."""
    def __init__(self, period: int, device, max_iter: Optional[int] = None):
        if int(period) < 1:
            raise ValueError("DeviceMetricRecorder: period must be >= 1")
        self.period, self.device, self.max_iter = int(period), torch.device(device), max_iter
        P = self.period
        self._words = P * (MAX_FLOATS + MAX_INTS + 1) + 1
        self._buf = torch.zeros(self._words, dtype=torch.int32, device=self.device)      # ring_f | ring_i | ring_iter | first_bad_iter
        o = P * MAX_FLOATS
        self.ring_f = self._buf[:o].view(torch.float32).view(P, MAX_FLOATS)
        self.ring_i = self._buf[o: o + P * MAX_INTS].view(P, MAX_INTS)
        self.ring_iter = self._buf[o + P * MAX_INTS: o + P * MAX_INTS + P]
        self.first_bad_iter = self._buf[self._words - 1:]
        self.ring_iter.fill_(-1)
        self.first_bad_iter.fill_(-1)
        self._mirror = torch.empty(self._words, dtype=torch.int32).pin_memory() if self.device.type == "cuda" else torch.empty(self._words, dtype=torch.int32)
        self.sink = HeadStatSink(self.device)
        self.keys: Tuple[str, ...] = ()
        self.suffixes: Tuple[str, ...] = ()
        self._count = 0                              # rows recorded since the last flush
        self._next = 0                               # next ring slot
        self._host: List[dict] = []                  # per recorded row: slot, iteration, images, data_time, time, lr
        self.storage: Optional[EventStorage] = None  # every flush puts its scalars here and hands them to the writers
        self.writers: list = []

    # -- one launch per iteration
    def record(self, loss_dict: Dict[str, torch.Tensor], counters: Optional[Sequence[torch.Tensor]] = None, iteration: int = 0,
               data_time: Optional[float] = None, images: Optional[Dict[str, int]] = None):
        """append the row of `iteration`: the values of loss_dict (0-d fp32 device tensors; key order = dict order) and the int32 counter
        words (default: the sink's, which are cleared by the launch).  A changed key set flushes the open window first.
        The engines publish their losses as fp32 device scalars, and those are recorded by address: one launch per iteration.  Any other
        value (a Python number, a tensor of another dtype or device) is first converted to one -- a slow path of one extra launch or
        host-to-device copy per such key and iteration, kept so that a foreign model's loss dict is logged rather than rejected."""
        own = counters is None
        if own:
            counters = self.sink.counter_tensors()
            images = dict(self.sink.images)
        keys, suffixes = tuple(loss_dict.keys()), tuple(self.sink.suffixes) if own else ()
        if len(keys) > MAX_FLOATS or len(counters) > MAX_INTS:
            raise ValueError(f"metrics: at most {MAX_FLOATS} loss keys and {MAX_INTS} counters per row, got {len(keys)} / {len(counters)}")
        if self._count and (keys != self.keys or suffixes != self.suffixes):
            self.flush()
        self.keys, self.suffixes = keys, suffixes
        src = []
        for v in loss_dict.values():
            if not (isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.device == self.device and v.numel() == 1):
                v = torch.as_tensor(v).detach().to(device=self.device, dtype=torch.float32).reshape(1)
            src.append(v.detach())
        slot = self._next
        self._launch(src, counters, slot, int(iteration), own)
        self._next = (slot + 1) % self.period
        self._count += 1
        self._host.append(dict(slot=slot, iteration=int(iteration), images=images or {}, data_time=data_time, time=None, lr=None))
        del self._host[:-self.period]

    def _launch(self, src, counters, slot: int, iteration: int, clear: bool):
        """the one launch of `record`: aldi_metrics_record on the current stream (stream order: behind the step's last loss, before the
        next iteration's counting launches, whose counters it clears, and before a flush's copy)"""
        from . import ops
        ops.metrics_record(src, counters, self.ring_f, self.ring_i, self.ring_iter, slot, iteration, self.first_bad_iter, clear_counters=clear)

    def note_step(self, time_s: Optional[float] = None, lr: Optional[float] = None):
        """host measurements of the row recorded last: seconds since the previous after_step, the learning rate of the step"""
        if self._host:
            self._host[-1].update(time=time_s, lr=lr)

    def pending(self) -> int:
        return min(self._count, self.period)

    # -- once per window
    def flush(self) -> Optional["OrderedDict[str, float]"]:
        """the open window's statistics (None: nothing recorded since the last flush) with `iteration` = its last row's, put into
        `storage` and handed to every writer; FloatingPointError when a recorded loss was not finite.  The host waits here for the
        device -- and nowhere else."""
        rows = self._host[-self.pending():] if self.pending() else []
        self._count, self._host = 0, []
        if not rows:
            return None
        P, nf, ns = self.period, len(self.keys), len(self.suffixes)
        slots = [r["slot"] for r in rows]
        times = np.array([[r["data_time"] if r["data_time"] is not None else np.nan, r["time"] if r["time"] is not None else np.nan] for r in rows])
        images = np.array([[r["images"].get(s, 0) for s in self.suffixes] for r in rows], dtype=np.float64).reshape(len(rows), ns)
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world > 1:
            idx = torch.tensor(slots, device=self.device)
            sums = torch.cat([self.ring_f[idx, :nf].double(), self.ring_i[idx, :ns * len(STAT_NAMES)].double(),
                              torch.from_numpy(images).to(self.device)], dim=1)
            # (the earliest bad iteration of any rank rides in the MAX reduction as its negative, so that every rank raises together)
            bad = torch.where(self.first_bad_iter >= 0, -self.first_bad_iter.double(), torch.full((1,), -float("inf"), dtype=torch.float64, device=self.device))
            maxes = torch.cat([torch.from_numpy(np.nan_to_num(times, nan=-1.0)).to(self.device).reshape(-1), bad])
            reduce_window(sums, nf, maxes, world)
            sums, maxes = sums.cpu().numpy(), maxes.cpu().numpy()          # (the host waits here)
            values, counts, images = sums[:, :nf], sums[:, nf: nf + ns * len(STAT_NAMES)], sums[:, nf + ns * len(STAT_NAMES):]
            times = maxes[:-1].reshape(len(rows), 2)
            times = np.where(times < 0, np.nan, times)
            first_bad = int(-maxes[-1]) if np.isfinite(maxes[-1]) else -1
        else:
            if self.device.type == "cuda":
                self._mirror.copy_(self._buf, non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()       # (the host waits here)
            else:
                self._mirror.copy_(self._buf)
            m = self._mirror.numpy()
            o = P * MAX_FLOATS
            values = m[:o].view(np.float32).reshape(P, MAX_FLOATS)[slots, :nf].astype(np.float64)
            counts = m[o: o + P * MAX_INTS].reshape(P, MAX_INTS)[slots, :ns * len(STAT_NAMES)].astype(np.float64)
            first_bad = int(m[-1])
        iteration = rows[-1]["iteration"]
        if first_bad >= 0:
            at = [i for i, r in enumerate(rows) if r["iteration"] == first_bad]
            row = {k: float(values[at[0], j]) for j, k in enumerate(self.keys)} if at else {}
            raise FloatingPointError(f"Loss became infinite or NaN at iteration={first_bad}!\nloss_dict = {row}")
        dt, tm = times[:, 0], times[:, 1]
        lrs = [r["lr"] for r in rows if r["lr"] is not None]
        stats = window_stats(self.keys, values, data_time=dt[~np.isnan(dt)], time=tm[~np.isnan(tm)], lr=lrs[-1] if lrs else None,
                             iteration=iteration, max_iter=self.max_iter, suffixes=self.suffixes, counts=counts, images=images)
        stats["iteration"] = iteration
        stats.move_to_end("iteration", last=False)
        if self.storage is not None:
            self.storage.iter = iteration
            self.storage.put_scalars(cur_iter=iteration, **{k: v for k, v in stats.items() if k != "iteration"})
        for w in self.writers:
            w.write(stats)
        return stats


# ------------------------------------------------------------------------------------------------ writers
class JSONWriter:
    """one JSON object per flush appended to `json_file`, `iteration` first; append mode, so a resumed run continues the file"""
    def __init__(self, json_file: str):
        d = os.path.dirname(json_file)
        if d:
            os.makedirs(d, exist_ok=True)
        self._path = json_file
        self._fh = open(json_file, "a")

    def write(self, stats: Dict[str, float]):
        row = OrderedDict(iteration=int(stats["iteration"]))
        row.update((k, v) for k, v in stats.items() if k != "iteration")
        self._fh.write(json.dumps(row) + "\n")
        self._fh.flush()                             # (to the OS: a killed run keeps its lines; no fsync -- a disk wait per window buys nothing here)

    def close(self):
        self._fh.close()


class CommonMetricPrinter:
    """one `logging` line per flush: eta, iter, total_loss, every key containing "loss", time, data_time, lr, max_mem"""
    def __init__(self, max_iter: Optional[int] = None):
        self.logger = logging.getLogger("aldi_amd.events")
        self._max_iter = max_iter

    def format(self, stats: Dict[str, float]) -> str:
        eta = stats.get("eta_seconds")
        parts = [" eta: {}".format(str(datetime.timedelta(seconds=int(eta))) if eta is not None else "N/A"), "iter: {}".format(int(stats["iteration"]))]
        if "total_loss" in stats:
            parts.append("total_loss: {:.4g}".format(stats["total_loss"]))
        parts += ["{}: {:.4g}".format(k, v) for k, v in stats.items() if "loss" in k and k != "total_loss"]
        for k in ("time", "data_time"):
            if k in stats:
                parts.append("{}: {:.4f}".format(k, stats[k]))
        if "lr" in stats:
            parts.append("lr: {:.5g}".format(stats["lr"]))
        if torch.cuda.is_available():
            parts.append("max_mem: {:.0f}M".format(torch.cuda.max_memory_allocated() / 1024.0 / 1024.0))
        return "  ".join(parts)

    def write(self, stats: Dict[str, float]):
        self.logger.info(self.format(stats))

    def close(self):
        pass

"""SOLVER.LOG_PERIOD on the device: the three kernels of csrc/trainstats.hip against torch-CPU formulas (exact integers / exact bits),
and the trainer's logging end to end -- metrics.json equals the numpy medians of the values the step published, the head statistics
equal detectron2's _log_classification_stats formulas on the engine's own tensors, logging does not disturb the step, and a
non-finite loss raises before anything is saved."""
import glob
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 192, 256
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ aldi_metrics_record
def _bits(values):
    return np.asarray(values, dtype=np.uint32).view(np.float32)


FINITE_SPECIALS = _bits([0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff, 0x00000000])      # -0.0, denormals, FLT_MAX, +0.0
NONFINITE = {5: _bits([0x7f800000])[0], 6: _bits([0xffc12345])[0], 7: _bits([0xff800000])[0]}      # +inf, a NaN with a payload, -inf
WINDOW = 4


def _record_inputs(K, with_bad):
    rng = np.random.RandomState(K)
    rows = 2 * WINDOW + 1
    v = rng.standard_normal((rows, K)).astype(np.float32)
    for t in range(rows):
        for j in range(min(K, 2)):
            v[t, (t + 3 * j) % K] = FINITE_SPECIALS[(t + j) % len(FINITE_SPECIALS)]
        if with_bad and t in NONFINITE:
            v[t, t % K] = NONFINITE[t]
    return v


@pytest.mark.parametrize("ni", [0, 16, 32])
@pytest.mark.parametrize("K", [1, 13, 64])
def test_record_copies_bits_wraps_and_flags_the_first_bad_iteration(K, ni):
    from aldi_amd import ops
    rows = 2 * WINDOW + 1
    for with_bad in (False, True):
        v = _record_inputs(K, with_bad)
        cnt = np.random.RandomState(ni + 1).randint(-2 ** 31, 2 ** 31 - 1, size=(rows, max(ni, 1)), dtype=np.int64).astype(np.int32)
        dv, dc = torch.from_numpy(v).to(DEV), torch.from_numpy(cnt).to(DEV)
        ring_f = torch.full((WINDOW, 64), 7.0, device=DEV)
        ring_i = torch.full((WINDOW, 32), 7, dtype=torch.int32, device=DEV)
        ring_it = torch.full((WINDOW,), -1, dtype=torch.int32, device=DEV)
        bad = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        exp_f = np.full((WINDOW, 64), 7.0, dtype=np.float32).view(np.int32).copy()
        exp_i = np.full((WINDOW, 32), 7, dtype=np.int32)
        exp_it = np.full((WINDOW,), -1, dtype=np.int32)
        exp_bad = -1
        for t in range(rows):
            slot, it = t % WINDOW, 100 + t
            ops.metrics_record([dv[t, j: j + 1] for j in range(K)], [dc[t, j: j + 1] for j in range(ni)], ring_f, ring_i, ring_it, slot, it, bad)
            exp_f[slot] = 0
            exp_f[slot, :K] = v[t].view(np.int32)
            exp_i[slot] = 0
            exp_i[slot, :ni] = cnt[t, :ni]
            exp_it[slot] = it
            if exp_bad < 0 and not np.isfinite(v[t]).all():
                exp_bad = it
            assert np.array_equal(ring_f.view(torch.int32).cpu().numpy(), exp_f), (t, with_bad)
            assert np.array_equal(ring_i.cpu().numpy(), exp_i) and np.array_equal(ring_it.cpu().numpy(), exp_it), t
            assert int(bad) == exp_bad, (t, int(bad), exp_bad)
        assert exp_bad == (105 if with_bad else -1)
        assert torch.equal(dc.cpu(), torch.from_numpy(cnt))              # (clear_counters off: the sources are only read)


def test_record_clears_the_counters_on_request_and_rejects_bad_arguments():
    from aldi_amd import _lib as L
    from aldi_amd import ops
    src = torch.arange(1, 8, dtype=torch.int32, device=DEV)
    ring_f = torch.zeros((2, 64), device=DEV)
    ring_i = torch.zeros((2, 32), dtype=torch.int32, device=DEV)
    ring_it = torch.zeros((2,), dtype=torch.int32, device=DEV)
    bad = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ops.metrics_record([], [src[j: j + 1] for j in range(5)], ring_f, ring_i, ring_it, 1, 9, bad, clear_counters=True)
    assert ring_i[1, :7].tolist() == [1, 2, 3, 4, 5, 0, 0] and src.tolist() == [0, 0, 0, 0, 0, 6, 7] and int(ring_it[1]) == 9 and int(bad) == -1
    with pytest.raises(L.AldiHipError):
        ops.metrics_record([], [], ring_f, ring_i, ring_it, 2, 0, bad)          # slot outside the ring
    one = torch.zeros(1, device=DEV)
    with pytest.raises(L.AldiHipError):
        ops.metrics_record([one] * 65, [], ring_f, ring_i, ring_it, 0, 0, bad)


# ------------------------------------------------------------------------------------------------ aldi_box_cls_stats
def _pad16(n):
    return (n + 15) // 16 * 16


def ref_box_stats(pred, cls, K):
    """detectron2 _log_classification_stats as counts, torch CPU ops: argmax over columns 0 .. K (a NaN counts as the maximum, the first
    maximum wins); foreground 0 <= cls < K"""
    s = pred[:, : K + 1].float()
    idx = torch.arange(K + 1).expand_as(s)
    nan = torch.isnan(s)
    first_nan = torch.where(nan, idx, torch.full_like(idx, K + 1)).min(dim=1).values
    clean = torch.where(nan, torch.full_like(s, float("-inf")), s)
    mx = clean.max(dim=1, keepdim=True).values
    first_max = torch.where(clean == mx, idx, torch.full_like(idx, K + 1)).min(dim=1).values
    p = torch.where(nan.any(dim=1), first_nan, first_max)
    cls = cls.long()
    fg = (cls >= 0) & (cls < K)
    return [int(cls.numel()), int((p == cls).sum()), int(fg.sum()), int(((p == cls) & fg).sum()), int(((p == K) & fg).sum())]


def _box_case(dtype, K, R, seed, all_background=False):
    g = torch.Generator().manual_seed(seed)
    Cp = _pad16(5 * K + 1)
    pred = torch.randn((R, Cp), generator=g).to(dtype)
    pred[:, K + 1:] = 1e30                                # the box deltas: never part of the argmax
    cls = torch.randint(0, K + 1, (R,), generator=g, dtype=torch.int32)
    for r in range(R):
        kind = r % 7
        a, b = sorted(torch.randperm(K + 1, generator=g)[:2].tolist())
        if kind == 0:                                     # the maximum tied between two classes (bf16 rounding gives such rows for free too)
            top = pred[r, : K + 1].float().max() + 1.0
            pred[r, a] = pred[r, b] = top.to(dtype)
            cls[r] = (a, b)[(r // 7) % 2]
        elif kind == 1:                                   # a NaN beats everything, +inf included
            pred[r, a], pred[r, b] = float("inf"), float("nan")
            cls[r] = (a, b)[(r // 7) % 2]
        elif kind == 2:                                   # two NaNs: the first one
            pred[r, a] = pred[r, b] = float("nan")
        elif kind == 3:
            pred[r, : K + 1] = float("-inf")              # every score -inf: column 0
        elif kind == 4:
            cls[r] = -1                                   # an ignored row is an instance, never foreground
        elif kind == 5:
            pred[r, a], pred[r, b] = 0.0, -0.0            # +0 == -0: a tie
            pred[r, : K + 1] = torch.minimum(pred[r, : K + 1].float(), torch.zeros(())).to(dtype)
    if all_background:
        cls[:] = K
    return pred, cls, Cp


def _ranges(R):
    cuts = [0, min(37, R), min(37, R), min(300, R), R]      # an empty range, ranges not aligned to 64
    return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 1)]


@pytest.mark.parametrize("R", [1, 63, 64, 65, 513])
@pytest.mark.parametrize("K", [1, 8, 80])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_box_cls_stats_equal_the_reference_counts(dtype, K, R):
    from aldi_amd import ops
    for all_bg in (False, True):
        pred, cls, Cp = _box_case(dtype, K, R, 1000 * K + R, all_background=all_bg)
        rng = _ranges(R)
        ref = [ref_box_stats(pred[a:b], cls[a:b], K) if b > a else [0] * 5 for a, b in rng]
        if all_bg:
            assert all(r[2] == 0 and r[3] == 0 and r[4] == 0 for r in ref)
        dp, dc = pred.to(DEV), cls.to(DEV)
        base = torch.arange(5 * len(rng), dtype=torch.int32).view(len(rng), 5)           # (+=: the words are not overwritten)
        out = base.to(DEV)
        for rep in (1, 2):                                # calling twice doubles the counts
            ops.box_cls_stats(dp, K, dc, [(a, b, out[i]) for i, (a, b) in enumerate(rng)])
            got = (out.cpu() - base).tolist()
            assert got == [[rep * x for x in r] for r in ref], (dtype, K, R, all_bg, rep, got, ref)
        whole = torch.zeros(5, dtype=torch.int32, device=DEV)
        ops.box_cls_stats(dp, K, dc, [(0, R, whole)])
        assert whole.tolist() == ref_box_stats(pred, cls, K)


# ------------------------------------------------------------------------------------------------ aldi_rpn_label_counts
@pytest.mark.parametrize("L_", [1, 255, 256, 257, 4099])
@pytest.mark.parametrize("N", [1, 3])
def test_rpn_label_counts_are_exact(N, L_):
    from aldi_amd import ops
    g = torch.Generator().manual_seed(N * 10000 + L_)
    for shift in (0, 1, 3):                               # a slice of a larger tensor: the first element is not 16-byte aligned
        flat = torch.randint(-1, 2, (N * L_ + 8,), generator=g, dtype=torch.int32)
        lab = flat[shift: shift + N * L_].view(N, L_)
        out = torch.tensor([7, 11], dtype=torch.int32, device=DEV)
        d = flat.to(DEV)[shift: shift + N * L_].view(N, L_)
        ops.rpn_label_counts(d, out)
        assert out.tolist() == [7 + int((lab == 1).sum()), 11 + int((lab == 0).sum())], (N, L_, shift)
        ops.rpn_label_counts(d, out)
        assert out.tolist() == [7 + 2 * int((lab == 1).sum()), 11 + 2 * int((lab == 0).sum())]


# ------------------------------------------------------------------------------------------------ the trainer
BASE_LR = 0.0002      # tests/test_step_graph_gpu.py's set-up with a tenth of its learning rate: at 0.002 the random-init run diverges within the
                      # 11 iterations used here (total loss 1e5 at iteration 10, then images without a sampled row), with logging or without


def _trainer(out_dir, log_period, graph=True, fused=True, max_iter=None, extra=()):
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.AMP.ENABLED", False, "SOLVER.BASE_LR", BASE_LR, "SOLVER.WARMUP_ITERS", 0, "SEED", 1,
                         "EMA.ALPHA", 0.9, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W, "SOLVER.LOG_PERIOD", log_period,
                         "OUTPUT_DIR", str(out_dir), "TEST.EVAL_PERIOD", 0] + list(extra))
    if max_iter is not None:
        cfg.SOLVER.MAX_ITER = max_iter
    cfg.SOLVER.FUSED_STEP = fused
    cfg.SOLVER.STEP_GRAPH = graph
    random.seed(4)
    torch.manual_seed(17)
    tr = ALDITrainer(cfg)
    saved = tr.saved = []
    tr.checkpointer.save = lambda name, **kw: saved.append(name)         # (no half-gigabyte files from a test about logging)
    return tr


def _step(tr, it):
    tr.iter = it
    tr.before_step()
    tr.run_step()
    tr.after_step()
    torch.cuda.synchronize()
    return {k: float(v) for k, v in tr._trainer.last_loss_dict.items()}


def _lines(out_dir):
    with open(os.path.join(str(out_dir), "metrics.json")) as f:
        return [json.loads(line) for line in f if line.strip()]


HEAD = ("fast_rcnn/cls_accuracy", "fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative", "roi_head/num_fg_samples", "roi_head/num_bg_samples",
        "rpn/num_pos_anchors", "rpn/num_neg_anchors")
NEEDS_FG = ("fast_rcnn/fg_cls_accuracy", "fast_rcnn/false_negative")


@pytest.mark.parametrize("fused", [True, False])
def test_metrics_json_holds_the_window_medians_of_the_published_losses(tmp_path, fused):
    tr = _trainer(tmp_path, 4, graph=True, fused=fused, max_iter=11)
    assert tr.metric_recorder is not None and tr.model.engine.stats_sink is tr.metric_recorder.sink
    kept = [_step(tr, it) for it in range(11)]
    if fused:
        fs = tr._trainer._fused_step
        assert fs.stats["replays_a"] >= 1 and fs.stats["replays_b"] >= 1, fs.stats       # the statistics launches were replayed, not only issued
    else:
        assert getattr(tr._trainer, "_fused_step", None) is None
    lines = _lines(tmp_path)
    assert [ln["iteration"] for ln in lines] == [3, 7, 10] and all(next(iter(ln)) == "iteration" for ln in lines)
    assert tr.saved == ["model_final"]
    windows = [range(0, 4), range(4, 8), range(8, 11)]
    loss_keys = list(kept[0])
    assert all(list(k) == loss_keys for k in kept) and "loss_cls_source_strong" in loss_keys and "loss_roih_l1_distill" in loss_keys
    all_head = {f"{h}_{s}" for h in HEAD for s in ("source_strong", "distill")}
    optional = {f"{h}_distill" for h in NEEDS_FG}           # (no pseudo-label survived the threshold in the whole window: no foreground row)
    for ln, win in zip(lines, windows):
        for k in loss_keys:
            assert ln[k] == float(np.median([kept[it][k] for it in win])), (ln["iteration"], k)
        totals = [sum(kept[it][k] for k in loss_keys) for it in win]
        assert ln["total_loss"] == float(np.median(totals))
        keys = set(ln)
        fixed = set(loss_keys) | {"total_loss", "data_time", "time", "lr", "eta_seconds", "iteration"}
        assert fixed <= keys and keys - fixed <= all_head and all_head - optional <= keys - fixed, sorted(keys ^ (fixed | all_head))
        assert ln["lr"] == BASE_LR and ln["time"] > 0 and ln["data_time"] >= 0
        assert ln["eta_seconds"] == ln["time"] * (11 - ln["iteration"] - 1)
        assert 0.0 <= ln["fast_rcnn/cls_accuracy_source_strong"] <= 1.0 and ln["roi_head/num_fg_samples_source_strong"] > 0
        assert ln["roi_head/num_fg_samples_source_strong"] + ln["roi_head/num_bg_samples_source_strong"] <= 512
        assert 0 < ln["rpn/num_pos_anchors_source_strong"] + ln["rpn/num_neg_anchors_source_strong"] <= 256
    # the storage saw the same scalars
    latest = tr.storage.latest()
    assert latest["total_loss"] == (lines[-1]["total_loss"], 10) and [it for _, it in tr.storage.history("total_loss")] == [3, 7, 10]


def _ref_head_stats(pred, cls, labels, K, images):
    n_inst, n_acc, n_fg, n_fg_acc, n_fn = ref_box_stats(pred, cls, K)
    pos, neg = int((labels == 1).sum()), int((labels == 0).sum())
    out = {"fast_rcnn/cls_accuracy": n_acc / n_inst, "roi_head/num_fg_samples": n_fg / images, "roi_head/num_bg_samples": (n_inst - n_fg) / images,
           "rpn/num_pos_anchors": pos / images, "rpn/num_neg_anchors": neg / images}
    if n_fg:
        out.update({"fast_rcnn/fg_cls_accuracy": n_fg_acc / n_fg, "fast_rcnn/false_negative": n_fn / n_fg})
    return out


def _fused_chunks(c):
    """per micro-step suffix: the rows / classes / labels / images of the fused step's chunks, from its context"""
    per = {}
    for ch in c.chunks:
        d = per.setdefault(ch["name"], dict(pred=[], cls=[], lab=[], images=0))
        d["pred"].append(c.pred[ch["r0"]: ch["r1"]].float().cpu())
        d["cls"].append(c.r_cls[ch["r0"]: ch["r1"]].cpu())
        d["lab"].append(c.rpn_labels[ch["n0"]: ch["n1"]].cpu())
        d["images"] += ch["n1"] - ch["n0"]
    return per


def _assert_head_keys(ln, per, K, it):
    for name, d in per.items():
        ref = _ref_head_stats(torch.cat(d["pred"]), torch.cat(d["cls"]), torch.cat(d["lab"]), K, d["images"])
        got = {h: ln[f"{h}_{name}"] for h in HEAD if f"{h}_{name}" in ln}
        assert got == ref, (it, name, got, ref)


@pytest.mark.parametrize("fused", [True, False])
def test_head_statistics_equal_the_reference_formulas_on_the_engines_tensors(tmp_path, fused):
    """eager launches (STEP_GRAPH off), LOG_PERIOD 1: each line is one iteration, so its head keys are that iteration's ratios"""
    tr = _trainer(tmp_path, 1, graph=False, fused=fused, max_iter=100)
    eng = tr.model.engine
    K = eng.K
    seen = []
    if not fused:                                            # the sequential driver: one student forward per micro-step, named by the sink
        forward_train = eng.forward_train

        def tapped(*a, **kw):
            name = eng.stats_sink.current
            c = forward_train(*a, **kw)
            seen.append((name, c))
            return c
        eng.forward_train = tapped
    for it in range(2):
        del seen[:]
        _step(tr, it)
        ln = _lines(tmp_path)[-1]
        assert ln["iteration"] == it
        if fused:
            per = _fused_chunks(tr.model._last_fused)
        else:
            per = {}
            for name, c in seen:
                d = per.setdefault(name, dict(pred=[], cls=[], lab=[], images=0))
                d["pred"].append(c.pred[: c.R].float().cpu())
                d["cls"].append(c.r_cls[: c.R].cpu())
                d["lab"].append(c.rpn_labels.cpu())
                d["images"] += c.N
        assert set(per) == {"source_strong", "distill"}
        _assert_head_keys(ln, per, K, it)


def test_sink_box_takes_more_ranges_than_one_launch_and_merges_a_micro_steps_chunks():
    """aldi_box_cls_stats takes 8 ranges per launch; a fused step has up to 16 chunks"""
    from aldi_amd import ops
    from aldi_amd.events import HeadStatSink
    K, R = 8, 23 * 17
    pred, cls, _ = _box_case(torch.float32, K, R, 77)
    dp, dc = pred.to(DEV), cls.to(DEV)
    names = ["a", "b", "c", "a", "a", "b", "c", "c", "c", "a", "b", "a", "c", "b", "b", "a", "c"]      # 17 ranges, 13 after merging
    ranges = [(n, 23 * i, 23 * (i + 1)) for i, n in enumerate(names)]
    launches = []
    box_cls_stats = ops.box_cls_stats
    ops.box_cls_stats = lambda p, k, c, rng: (launches.append(len(rng)), box_cls_stats(p, k, c, rng))[1]
    try:
        sink = HeadStatSink(DEV)
        sink.box(dp, K, dc, ranges + [("b", 5, 5)])
    finally:
        ops.box_cls_stats = box_cls_stats
    assert launches == [8, 5]
    for n in "abc":
        ref = [0] * 5
        for m, r0, r1 in ranges:
            if m == n:
                ref = [x + y for x, y in zip(ref, ref_box_stats(pred[r0:r1], cls[r0:r1], K))]
        assert sink.words(n)[:5].tolist() == ref and sink.words(n)[5:].tolist() == [0, 0], n


def test_fused_step_with_more_than_eight_chunks_logs_its_head_statistics(tmp_path):
    """IMS_PER_GPU 1 with 5 + 5 images: ten chunks in one fused pass (the box losses then run per chunk), eager steps and replayed ones"""
    tr = _trainer(tmp_path, 1, graph=True, fused=True, max_iter=100, extra=["SOLVER.IMS_PER_BATCH", 10, "SOLVER.IMS_PER_GPU", 1])
    K = tr.model.engine.K
    for it in range(5):
        _step(tr, it)
        c = tr.model._last_fused
        assert len(c.chunks) == 10 and [ch["name"] for ch in c.chunks] == ["source_strong"] * 5 + ["distill"] * 5
        ln = _lines(tmp_path)[-1]
        assert ln["iteration"] == it
        per = _fused_chunks(c)
        assert per["source_strong"]["images"] == 5 and per["distill"]["images"] == 5
        _assert_head_keys(ln, per, K, it)
    fs = tr._trainer._fused_step
    assert fs.stats["eager"] == 3 and fs.stats["replays_b"] == 2, fs.stats


def _copy_state(src, dst):
    """as tests/test_step_graph_gpu.py: dst starts its next iteration from exactly src's state"""
    for a, b in ((src.model, dst.model), (src.ema.model, dst.ema.model)):
        b.weights.master.copy_(a.weights.master)
        b.weights.refresh()
    dst.model.weights.mom.copy_(src.model.weights.mom)
    dst.model.weights.first_step = src.model.weights.first_step
    dst._trainer.distiller.seeder.seed = src._trainer.distiller.seeder.seed
    dst.scheduler.last_iter = src.scheduler.last_iter
    dst.scheduler._apply()


def test_logging_does_not_disturb_the_step(tmp_path):
    a, b = _trainer(tmp_path / "a", 0), _trainer(tmp_path / "b", 4)
    assert a.metric_recorder is None and a._trainer.metric_recorder is None and a.model.engine.stats_sink is None
    assert a.ema.model.engine.stats_sink is None and b.ema.model.engine.stats_sink is None      # (the teacher computes no losses)
    assert b.model.engine.stats_sink is b.metric_recorder.sink
    for it in range(5):
        _copy_state(a, b)
        rng, py = torch.get_rng_state(), random.getstate()
        _step(a, it)
        rng_a, py_a = torch.get_rng_state(), random.getstate()
        torch.set_rng_state(rng)
        random.setstate(py)
        _step(b, it)
        assert torch.equal(torch.get_rng_state(), rng_a) and random.getstate() == py_a
        ca, cb = a.model._last_fused, b.model._last_fused
        assert torch.equal(ca.rpn_labels, cb.rpn_labels) and torch.equal(ca.r_idx[: ca.R], cb.r_idx[: cb.R]) and ca.rows == cb.rows
    assert not os.path.exists(os.path.join(str(tmp_path / "a"), "metrics.json"))
    assert [ln["iteration"] for ln in _lines(tmp_path / "b")] == [3]


# ------------------------------------------------------------------------------------------------ the non-finite guard
def _stub_trainer(out_dir, bad_at, checkpoint_period, max_iter=12):
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.trainer import DefaultTrainer
    values = torch.rand((max_iter, 2)) + 0.5
    values[bad_at, 1] = float("inf")
    dev_values = values.to(DEV)

    class Model:
        training = True
        device = torch.device(DEV)

        def __init__(self):
            self.p = torch.zeros((), device=DEV, requires_grad=True)
            self.calls = 0

        def __call__(self, data):
            row = dev_values[self.calls]
            self.calls += 1
            return {"loss_a": self.p * 0 + row[0], "loss_b": self.p * 0 + row[1]}

    class Optimizer:
        param_groups = [{"lr": 0.1}]

        def zero_grad(self, set_to_none=False):
            pass

        def step(self):
            pass

    class Checkpointer:
        def save(self, name, **kw):
            with open(os.path.join(str(out_dir), name + ".pth"), "w") as f:
                f.write(str(kw.get("iteration")))

    class Stub(DefaultTrainer):
        @classmethod
        def build_model(cls, cfg):
            return Model()

        @classmethod
        def build_optimizer(cls, cfg, model):
            return Optimizer()

        @classmethod
        def build_train_loader(cls, cfg):
            return iter(lambda: [{}], None)

        def create_ddp_model(self, model, broadcast_buffers, cfg):
            return model

        def _create_checkpointer(self, model, cfg):
            return Checkpointer()

    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_list(["SOLVER.LOG_PERIOD", 4, "SOLVER.CHECKPOINT_PERIOD", checkpoint_period, "SOLVER.MAX_ITER", max_iter, "OUTPUT_DIR", str(out_dir)])
    return Stub(cfg), values


def test_non_finite_loss_raises_before_the_checkpoint(tmp_path):
    tr, values = _stub_trainer(tmp_path, bad_at=5, checkpoint_period=6)
    with pytest.raises(FloatingPointError, match=r"Loss became infinite or NaN at iteration=5!\nloss_dict = ") as e:
        tr.train()
    assert "inf" in str(e.value) and "loss_b" in str(e.value)
    assert tr.iter == 5                                       # the flush in front of `model_0000005`
    assert glob.glob(os.path.join(str(tmp_path), "*.pth")) == []
    lines = _lines(tmp_path)
    assert [ln["iteration"] for ln in lines] == [3]
    assert lines[0]["loss_a"] == float(np.median(values[:4, 0].double().numpy()))


def test_non_finite_loss_is_reported_at_the_window_end_with_its_own_iteration(tmp_path):
    """no checkpoint in between: the flush of the window that holds iteration 5 comes LOG_PERIOD - 1 - (5 % LOG_PERIOD) iterations later"""
    tr, _ = _stub_trainer(tmp_path, bad_at=5, checkpoint_period=100)
    with pytest.raises(FloatingPointError, match=r"at iteration=5!"):
        tr.train()
    assert tr.iter == 7 and glob.glob(os.path.join(str(tmp_path), "*.pth")) == []

"""The host-only parts of the fused step (aldi_amd/fused_step.py): the chunk planner, the table of environment switches, the declared
per-shape state and the eviction of prefix slots.  No GPU: plain dicts with small uint8 tensors as images."""
import ast
import dataclasses
import os
from types import SimpleNamespace

import pytest
import torch

from aldi_amd import fused_step as F
from aldi_amd.trainer import plan_micro_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DA = (0.25, 0.5)


def _labeled(n):
    return [{"image": torch.zeros((3, 8, 8), dtype=torch.uint8), "instances": {"gt_boxes": torch.zeros((1, 4)), "gt_classes": torch.zeros(1, dtype=torch.long)}}
            for _ in range(n)]


def _unlabeled(n):
    return [{"image": torch.zeros((3, 8, 8), dtype=torch.uint8)} for _ in range(n)]


def _plan(lw, ls, uw, us, bs, do_align, do_distill):
    return F.plan_chunks(plan_micro_steps(lw, ls, uw, us, do_align=do_align, do_distill=do_distill), bs, DA)


def _layout(sp):
    return [(ch["name"], ch["n0"], ch["n1"]) for ch in sp.chunks]


def test_planner_shipped_per_gpu_batch():
    ls, uw, us = _labeled(6), _unlabeled(6), _unlabeled(6)
    sp = _plan(None, ls, uw, us, 2, do_align=False, do_distill=True)
    assert _layout(sp) == [("source_strong", 0, 2), ("source_strong", 2, 4), ("source_strong", 4, 6), ("distill", 6, 8), ("distill", 8, 10), ("distill", 10, 12)]
    assert [ch["kind"] for ch in sp.chunks] == ["labeled"] * 3 + ["distill"] * 3
    assert [ch.get("kd") for ch in sp.chunks] == [None, None, None, 0, 1, 2]
    assert all("kd" not in ch for ch in sp.chunks[:3])
    assert not any(ch["do_align"] for ch in sp.chunks) and all(ch["da_weights"] == DA for ch in sp.chunks)
    assert all(ch["labeled"] for ch in sp.chunks)
    assert (sp.N, sp.d0, sp.nk) == (12, 6, 3)
    assert len(sp.images) == 12 and all(a is b["image"] for a, b in zip(sp.images, ls + us))
    assert [i for i, _ in sp.lab_rows] == list(range(6))
    assert all(rec["gt_boxes"] is d["instances"]["gt_boxes"] for (_, rec), d in zip(sp.lab_rows, ls))


def test_planner_alignment_on():
    ls, uw, us = _labeled(2), _unlabeled(2), _unlabeled(2)
    sp = _plan(None, ls, uw, us, 2, do_align=True, do_distill=True)
    assert _layout(sp) == [("source_strong", 0, 2), ("target_weak", 2, 4), ("distill", 4, 6)]
    src, tgt, dst = sp.chunks
    assert src["kind"] == "labeled" and src["do_align"] is True
    assert tgt["kind"] == "unlabeled" and tgt["do_align"] is True and tgt["labeled"] is False
    assert tgt["keep"]("loss_da_img") and tgt["keep"]("x_da_y") and not tgt["keep"]("loss_cls") and not tgt["keep"]("loss_rpn_loc")
    assert dst["kind"] == "distill" and dst["do_align"] is False and dst["kd"] == 0
    assert (sp.N, sp.d0, sp.nk) == (6, 4, 1)
    assert all(a is b["image"] for a, b in zip(sp.images, ls + uw + us))          # the target_weak chunk runs the WEAK views
    assert [i for i, _ in sp.lab_rows] == [0, 1]


def test_planner_without_distillation():
    sp = _plan(None, _labeled(4), _unlabeled(4), _unlabeled(4), 2, do_align=False, do_distill=False)
    assert _layout(sp) == [("source_strong", 0, 2), ("source_strong", 2, 4)]
    assert sp.d0 == sp.N == 4 and sp.nk == 0


def test_planner_partial_last_micro_batch():
    sp = _plan(None, _labeled(3), None, None, 2, do_align=False, do_distill=False)
    assert _layout(sp) == [("source_strong", 0, 2), ("source_strong", 2, 3)]
    assert [i for i, _ in sp.lab_rows] == [0, 1, 2] and sp.N == 3


def test_planner_teacher_student_length_mismatch():
    with pytest.raises(AssertionError, match="Teacher and student data must be the same length"):
        _plan(None, _labeled(2), _unlabeled(2), _unlabeled(3), 2, do_align=False, do_distill=True)


def _cfg(**solver):
    return SimpleNamespace(SOLVER=dict(solver))


ENV = {"graph": "ALDI_STEP_GRAPH", "graph_b": "ALDI_STEP_GRAPH_B", "graph_flat": "ALDI_STEP_GRAPH_FLAT", "pair_forward": "ALDI_PAIR_FORWARD",
       "teacher_first": "ALDI_TEACHER_FIRST", "interleave": "ALDI_INTERLEAVE", "spin_wait": "ALDI_SPIN_WAIT", "pipeline": "ALDI_PIPELINE_PREFIX",
       "prefix_at": "ALDI_PREFIX_AT", "prefix_prio": "ALDI_PREFIX_PRIO", "main_prio": "ALDI_MAIN_PRIO", "sgd_stream": "ALDI_SGD_STREAM",
       "probe_spin_cycles": "ALDI_PROBE_SPIN_CYCLES", "housekeeping_late": "ALDI_HOUSEKEEPING_LATE", "rpn_loss_early": "ALDI_RPN_LOSS_EARLY",
       "rng_script": "ALDI_HOST_RNG_SCRIPT", "rng_prefetch": "ALDI_HOST_RNG_PREFETCH", "draws_c": "ALDI_HOST_DRAWS_C",
       "draws_rehearsal": "ALDI_HOST_DRAWS_REHEARSAL"}
# (variable value, the field's value then): each the opposite of the default
FLIPPED = {"graph": ("0", False), "graph_b": ("0", False), "graph_flat": ("0", False), "pair_forward": ("1", True), "teacher_first": ("1", True),
           "interleave": ("0", False), "spin_wait": ("0", False), "pipeline": ("1", True), "prefix_at": ("a", "a"), "prefix_prio": ("-1", -1),
           "main_prio": ("-1", -1), "sgd_stream": ("0", False), "probe_spin_cycles": ("2000", 2000), "housekeeping_late": ("0", False),
           "rpn_loss_early": ("0", False), "rng_script": ("0", False), "rng_prefetch": ("0", False), "draws_c": ("0", False), "draws_rehearsal": ("0", False)}


def test_knobs_defaults_with_an_empty_environment():
    k = F.StepKnobs.from_env(_cfg(), env={})
    assert k.graph is True and k.graph_b is True and k.graph_flat is True
    assert k.pair_forward is False and k.teacher_first is False and k.interleave is True
    assert k.spin_wait is True
    assert k.pipeline is False and k.prefix_at == "b" and k.prefix_prio == 0
    assert k.main_prio == 0
    assert k.sgd_stream is True
    assert k.probe_spin_cycles == 0
    assert k.housekeeping_late is True and k.rpn_loss_early is True
    assert k.rng_script is True and k.rng_prefetch is True and k.draws_c is True and k.draws_rehearsal is True
    assert set(ENV) == {f.name for f in dataclasses.fields(F.StepKnobs)}                 # the 19 switches, no more
    assert F.StepKnobs.from_env(_cfg(STEP_GRAPH=False), env={}).graph is False and F.StepKnobs.from_env(_cfg(PIPELINE_PREFIX=True), env={}).pipeline is True


@pytest.mark.parametrize("name", sorted(ENV))
def test_knob_variable_flips_exactly_its_field(name):
    base = F.StepKnobs.from_env(_cfg(), env={})
    raw, want = FLIPPED[name]
    k = F.StepKnobs.from_env(_cfg(), env={ENV[name]: raw})
    assert getattr(k, name) == want and getattr(k, name) != getattr(base, name)
    assert {f.name for f in dataclasses.fields(F.StepKnobs) if getattr(k, f.name) != getattr(base, f.name)} == {name}


def test_knobs_are_read_from_the_process_environment_and_frozen(monkeypatch):
    monkeypatch.setenv("ALDI_PAIR_FORWARD", "1")
    monkeypatch.delenv("ALDI_INTERLEAVE", raising=False)
    k = F.StepKnobs.from_env(_cfg())
    assert k.pair_forward is True and k.interleave is True
    with pytest.raises(AttributeError):
        k.pair_forward = False


def test_pipelining_request(monkeypatch):
    monkeypatch.setenv("ALDI_PIPELINE_PREFIX", "0")
    assert F.pipeline_prefix_requested(_cfg(PIPELINE_PREFIX=True)) is False and F.StepKnobs.from_env(_cfg(PIPELINE_PREFIX=True)).pipeline is False
    monkeypatch.setenv("ALDI_PIPELINE_PREFIX", "1")
    assert F.pipeline_prefix_requested(_cfg(PIPELINE_PREFIX=False)) is True and F.StepKnobs.from_env(_cfg(PIPELINE_PREFIX=False)).pipeline is True
    monkeypatch.delenv("ALDI_PIPELINE_PREFIX")
    assert F.pipeline_prefix_requested(_cfg(PIPELINE_PREFIX=True)) is True and F.pipeline_prefix_requested(_cfg()) is False


def test_environment_is_read_in_one_place_only():
    """`os.environ` occurs in aldi_amd/fused_step.py only inside StepKnobs.from_env (a plain text search of that file for that string)"""
    path = os.path.join(ROOT, "aldi_amd", "fused_step.py")
    with open(path) as f:
        src = f.read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "StepKnobs")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "from_env")
    hits = [i for i, line in enumerate(src.split("\n"), 1) if "os.environ" in line]
    assert hits and all(fn.lineno <= i <= fn.end_lineno for i in hits), hits
    assert "getattr(S," not in src


def test_per_shape_state_rejects_undeclared_names():
    S = F._ShapeState()
    S.N, S.chunk_arr = 4, None                                                 # declared
    assert S.prev_counts is None and S.pipe is False and S.bufs == {} and S.graphs_b == {}
    with pytest.raises(AttributeError):
        S.chunk_ar = None
    with pytest.raises(AttributeError):
        S.undeclared
    b = F._Batch(img=None, hw=None, key=(0, 1, 32, 32))
    with pytest.raises(AttributeError):
        b.size = None


def test_prefix_slots_leave_with_their_shapes():
    """more than 8 distinct shapes: `static` keeps the 8 most recent, and `_pslots` holds no slot (either parity) whose shape no remaining
    state uses; `_pre_ready` does not outlive its slot"""
    fs = F.FusedStep(SimpleNamespace(model=SimpleNamespace(cfg=_cfg())))
    for i in range(12):
        shape = (4, 32 * (i + 1), 64)
        for par in (0, 1):
            S = fs._static_for(("layout", shape, ("pipe", par)))
            S.pshape = shape
            for p in (0, 1):
                fs._pslots.setdefault((p,) + shape, F._Batch(img=None, hw=None, key=(p,) + shape))
        if i == 0:
            fs._pre_ready = (fs._pslots[(1,) + shape], [])
        live = {S.pshape for S in fs.static.values()}
        assert len(fs.static) <= 8 and {k[1:] for k in fs._pslots} <= live | {shape}, i
        if i < 4:
            assert fs._pre_ready is not None                                  # (8 states = 4 shapes x 2 parities: nothing dropped yet)
    assert len(fs.static) == 8 and len(fs._pslots) == 8 and {k[1:] for k in fs._pslots} == {S.pshape for S in fs.static.values()}
    assert fs._pre_ready is None
    # a shape two states share (EMA copy -> lerp) keeps its slots until the last of them goes
    fs = F.FusedStep(SimpleNamespace(model=SimpleNamespace(cfg=_cfg())))
    shared = (4, 32, 64)
    for tag in ("copy", "lerp"):
        fs._static_for((tag, shared)).pshape = shared
    fs._pslots[(0,) + shared] = F._Batch(img=None, hw=None, key=(0,) + shared)
    for i in range(7):
        fs._static_for(("other", i))
    assert ("copy", shared) not in fs.static and ("lerp", shared) in fs.static and (0,) + shared in fs._pslots
    fs._static_for(("other", 7))
    assert ("lerp", shared) not in fs.static and not fs._pslots

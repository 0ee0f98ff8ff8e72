"""The engine's table of environment switches (aldi_amd/engine.py: EngineKnobs) and RCNN.with_knobs.  No GPU."""
import ast
import dataclasses
import glob
import os
import re

import pytest

from aldi_amd.engine import RCNN, EngineKnobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENV = {"fused_stem": "ALDI_FUSED_STEM", "fused_res2": "ALDI_FUSED_RES2", "fused_res2_shortcut": "ALDI_FUSED_RES2_SHORTCUT",
       "fused_stage_entrance": "ALDI_FUSED_STAGE_ENTRANCE", "level_groups": "ALDI_LEVEL_GROUPS", "mask_bits": "ALDI_MASK_BITS",
       "mask_bits_inner": "ALDI_MASK_BITS_INNER", "mask_bits_fc": "ALDI_MASK_BITS_FC", "roi_prepare_fused": "ALDI_ROI_PREPARE_FUSED",
       "box_loss_fused": "ALDI_BOX_LOSS_FUSED", "sparse_rpn_backward": "ALDI_RPN_SPARSE_BWD", "upsample_chain": "ALDI_UPSAMPLE_CHAIN",
       "aux_stream": "ALDI_AUX_STREAM", "wgrad_stream": "ALDI_WGRAD_STREAM", "wgrad_prio": "ALDI_WGRAD_PRIO", "group_wgrad": "ALDI_WGRAD_GROUP",
       "wgrad_tail_split": "ALDI_WGRAD_TAIL_SPLIT", "wgrad_subsample": "ALDI_WGRAD_SUBSAMPLE", "wgrad_subsample_side": "ALDI_WGRAD_SUBSAMPLE_SIDE",
       "wgrad_bias_fused": "ALDI_WGRAD_BIAS_FUSED"}
INTS = {"wgrad_prio": ("-1", -1), "wgrad_tail_split": ("0", 0)}            # (variable value, the field's value then); every other switch is on: "0" -> False


def test_knobs_defaults_with_an_empty_environment():
    k = EngineKnobs.from_env(env={})
    assert k == EngineKnobs()
    assert k.wgrad_prio == 0 and k.wgrad_tail_split == 2
    assert all(getattr(k, name) is True for name in ENV if name not in INTS)
    assert set(ENV) == {f.name for f in dataclasses.fields(EngineKnobs)}                # the engine's switches, no more
    assert {f.name: f.metadata["env"] for f in dataclasses.fields(EngineKnobs)} == ENV
    assert all(f.metadata["doc"] for f in dataclasses.fields(EngineKnobs))


@pytest.mark.parametrize("name", sorted(ENV))
def test_knob_variable_flips_exactly_its_field(name):
    base = EngineKnobs.from_env(env={})
    raw, want = INTS.get(name, ("0", False))
    k = EngineKnobs.from_env(env={ENV[name]: raw})
    assert getattr(k, name) == want and type(getattr(k, name)) is type(want) and getattr(k, name) != getattr(base, name)
    assert {f.name for f in dataclasses.fields(EngineKnobs) if getattr(k, f.name) != getattr(base, f.name)} == {name}


def test_bool_knobs_are_on_for_the_string_1_only():
    assert EngineKnobs.from_env(env={"ALDI_FUSED_STEM": "1"}).fused_stem is True
    for raw in ("0", "", "true", "2"):
        assert EngineKnobs.from_env(env={"ALDI_FUSED_STEM": raw}).fused_stem is False


def test_knobs_are_read_from_the_process_environment_and_frozen(monkeypatch):
    monkeypatch.setenv("ALDI_UPSAMPLE_CHAIN", "0")
    monkeypatch.delenv("ALDI_LEVEL_GROUPS", raising=False)
    k = EngineKnobs.from_env()
    assert k.upsample_chain is False and k.level_groups is True
    with pytest.raises(AttributeError):
        k.upsample_chain = True


def _engine_source():
    with open(os.path.join(ROOT, "aldi_amd", "engine.py")) as f:
        return f.read()


def test_environment_is_read_in_one_place_only():
    """`os.environ` occurs in aldi_amd/engine.py only inside EngineKnobs.from_env (a plain text search of that file for that string)"""
    src = _engine_source()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "EngineKnobs")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "from_env")
    hits = [i for i, line in enumerate(src.split("\n"), 1) if "os.environ" in line or "getenv" in line]
    assert hits and all(fn.lineno <= i <= fn.end_lineno for i in hits), hits


def test_every_knob_is_connected():
    """every field is read as `knobs.<name>` somewhere in aldi_amd/*.py outside the table itself (a switch nobody reads is disconnected)"""
    src = _engine_source()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "EngineKnobs")
    lines = src.split("\n")
    text = "\n".join(lines[:cls.lineno - 1] + lines[cls.end_lineno:])
    for path in sorted(glob.glob(os.path.join(ROOT, "aldi_amd", "*.py"))):
        if os.path.basename(path) != "engine.py":
            with open(path) as f:
                text += "\n" + f.read()
    missing = [name for name in ENV if not re.search(r"knobs\." + name + r"\b", text)]
    assert not missing, missing


def test_with_knobs_restores_the_table_after_an_exception():
    m = RCNN.__new__(RCNN)                                   # (no device: only the table is touched)
    m.knobs = old = EngineKnobs.from_env(env={})
    with m.with_knobs(level_groups=False, wgrad_tail_split=0) as inner:
        assert inner is m and m.knobs.level_groups is False and m.knobs.wgrad_tail_split == 0 and m.knobs.mask_bits is True
        assert m.sparse_rpn_backward is True
        with m.with_knobs(sparse_rpn_backward=False):
            assert m.sparse_rpn_backward is False and m.knobs.level_groups is False
        assert m.sparse_rpn_backward is True
    assert m.knobs is old
    with pytest.raises(ZeroDivisionError):
        with m.with_knobs(level_groups=False):
            1 / 0
    assert m.knobs is old
    with pytest.raises(TypeError):
        with m.with_knobs(no_such_switch=1):
            pass
    assert m.knobs is old
    with pytest.raises(AttributeError):
        m.sparse_rpn_backward = False                        # read-only: the table is the one place a switch lives

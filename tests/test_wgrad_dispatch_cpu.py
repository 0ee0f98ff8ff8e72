"""What a weight-gradient call launches, checked without a GPU: aldi_conv_wgrad_plan (the dry run of aldi_conv_wgrad / aldi_conv_wgrad_group:
csrc/wgrad_select.h) against tests/golden/wgrad_dispatch_table.json, which tools/record_wgrad_dispatch.py recorded from real launches
(aldi_last_dispatch() after each, aldi_conv_wgrad_group_workspace before) BEFORE the plan was separated from the launch.  A threshold or
rule edit shows here as the rows it moves."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "wgrad_dispatch_table.json")
DUMMY = 0x10000          # a non-null address: the plan never dereferences it
BIG_WS = 1 << 40         # (the recorder passed one workspace sized for the whole sweep)


def _tool():
    spec = importlib.util.spec_from_file_location("record_wgrad_dispatch", os.path.join(ROOT, "tools", "record_wgrad_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        rows = json.load(f)
    assert len(rows) > 1000
    return rows


@pytest.fixture(autouse=True)
def _reset_tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


PTR = {f: DUMMY for f in ("x", "g", "dw", "db", "scale", "ws")}


def _args(L, T, case, knobs, ws_bytes=BIG_WS):
    L.reset_tuning()
    for k, v in knobs.items():
        L.set_tuning(k, v)
    return T.wgrad_args(L, case, PTR, ws_bytes)


def test_plan_reproduces_every_recorded_row(table):
    from aldi_amd import _lib as L
    T = _tool()
    bad = []
    for case, knobs, name, ws in table:
        arr = _args(L, T, case, knobs)
        got = L.plan_wgrad_dispatch(arr, len(case) - 1, case[0] == "g")
        query = L.lib.aldi_conv_wgrad_group_workspace(arr, len(case) - 1)
        if got != (name, ws) or query != ws:
            bad.append((case, knobs, name, ws, got, query))
    assert not bad, (len(bad), bad[:5])


def _key(case, knobs):
    return json.dumps([case, knobs], sort_keys=True)


def test_recorded_rows_agree_with_the_names_the_gpu_tests_assert(table):
    """a bad recording cannot go unnoticed: rows looked up by (shapes, operands, knobs) against the literal strings of tests/test_dispatch_gpu.py"""
    T = _tool()
    by_key = {_key(case, knobs): name for case, knobs, name, _ in table}

    def single(dt, shape, knobs=None, flags=None):
        return by_key[_key(["s", T.prob(dt, shape, flags or ("scale+ws" if dt == "bf16" else "scale"))], knobs or {})]

    def kernel(*a, **kw):
        return single(*a, **kw).split(" ")[0]

    def group(shapes, knobs=None, flags="scale+db+ws"):
        return by_key[_key(["g"] + [T.prob("bf16", s, flags) if isinstance(s, tuple) else s for s in shapes], knobs or {})]

    # test_wgrad_fullsize_default_dispatch
    for shape, expect in [((4, 200, 336, 256, 256, 3, 1, 1), "wgrad_bf16_big64"), ((4, 100, 168, 256, 256, 3, 1, 1), "wgrad_bf16_big64"),
                          ((4, 200, 336, 256, 256, 1, 1, 0), "wgrad_bf16_lean"), ((4, 50, 84, 256, 256, 3, 1, 1), "wgrad_bf16_lean"),
                          ((4, 50, 84, 1024, 256, 1, 1, 0), "wgrad_bf16_lean"), ((4, 100, 168, 128, 512, 1, 1, 0), "wgrad_bf16_lean"),
                          ((4, 200, 336, 256, 512, 1, 2, 0), "wgrad_bf16_generic"), ((2048, 1, 1, 12544, 1024, 1, 1, 0), "wgrad_bf16_big64"),
                          ((4, 200, 336, 256, 16, 1, 1, 0), "wgrad_bf16_lean"), ((2, 200, 336, 256, 256, 3, 1, 0), "wgrad_bf16_generic")]:
        assert kernel("bf16", shape) == expect, shape
        assert single("bf16", shape).endswith(" ordered") == (expect != "wgrad_bf16_generic") and " ordered" not in single("bf16", shape, flags="scale")
    # test_wgrad_forced_big_and_generic_small
    for shape in T.SMALL:
        big_ok = shape[4] % 256 == 0 and (shape[5] ** 2 * shape[3]) % 256 == 0
        assert kernel("bf16", shape, {"wgrad_big_min": 1, "wgrad_big_slots": 2}) == ("wgrad_bf16_big64" if big_ok else "wgrad_bf16_lean"), shape
        assert kernel("bf16", shape, {"wgrad_big_min": 0}) == "wgrad_bf16_lean"
        assert kernel("bf16", shape, {"wgrad_lean": 0}) == "wgrad_bf16_generic"
        assert kernel("f32", shape) == "wgrad_f32_t128" and kernel("f32", shape, {"wgrad_f32_tile128": 0}) == "wgrad_f32"
    # test_wgrad_split_count_does_not_change_the_result, test_wgrad_dma_split_counts
    for slots in (1, 64, 1000):
        assert kernel("bf16", T.SPLIT_CASE, {"wgrad_slots": slots, "wgrad_big_min": 0}) == "wgrad_bf16_lean"
        assert kernel("bf16", T.SPLIT_CASE, {"wgrad_big_slots": slots, "wgrad_big_min": 1}) == "wgrad_bf16_big64"
        assert kernel("bf16", T.SPLIT_CASE, {"wgrad_dma": 2, "wgrad_slots": slots}) == "wgrad_bf16_dma"
    assert single("bf16", T.SPLIT_CASE, {"wgrad_slots": 1, "wgrad_big_min": 0}) == "wgrad_bf16_lean splits=1 ordered"
    assert single("bf16", T.SPLIT_CASE, {"wgrad_slots": 64, "wgrad_big_min": 0}) == "wgrad_bf16_lean splits=2 ordered"          # 36 tiles
    assert single("bf16", T.SPLIT_CASE, {"wgrad_slots": 1000, "wgrad_big_min": 0}) == "wgrad_bf16_lean splits=27 ordered"       # 132 slabs, 5 each
    # test_wgrad_big_tile_register_staged_arm
    for shape in T.BIG_ARM:
        assert kernel("bf16", shape, {"wgrad_dma64": 0, "wgrad_big_min": 1, "wgrad_big_slots": 8}) == "wgrad_bf16_big"
        assert kernel("bf16", shape, {"wgrad_dma64": 1, "wgrad_big_min": 1, "wgrad_big_slots": 8}) == "wgrad_bf16_big64"
    # test_wgrad_fp32_fullsize, test_wgrad_fp32_dispatch_and_values
    for shape, expect in zip(T.F32_CASES, ["wgrad_f32_t128", "wgrad_f32_t128", "wgrad_f32_t128", "wgrad_f32", "wgrad_f32_t128", "wgrad_f32_t128", "wgrad_f32"]):
        assert kernel("f32", shape) == expect, shape
    assert kernel("f32", T.F32_CASES[0], {"wgrad_f32_tile128": 0}) == "wgrad_f32"
    # test_wgrad_dma_kernel
    for shape in T.DMA_CASES:
        assert kernel("bf16", shape, {"wgrad_dma": 2}) == "wgrad_bf16_dma", shape
    # test_bias_gradient_rides_in_the_wgrad_launch
    for shape, expect in zip(T.BIAS_CASES, ["wgrad_bf16_lean", "wgrad_bf16_lean", "wgrad_bf16_big64", "wgrad_bf16_generic"]):
        assert kernel("bf16", shape, flags="db+ws") == expect, shape
    assert kernel("f32", (1, 25, 42, 64, 64, 3, 1, 1), flags="db") == "wgrad_f32"
    # test_wgrad_group_register_staged_loops, test_wgrad_interleaved_loop_equals_lockstep_bit_for_bit
    assert "64_group" in group(T.G_LOOPS) and "_group" in group(T.G_LOOPS, {"wgrad_dma64": 0}) and "64_group" not in group(T.G_LOOPS, {"wgrad_dma64": 0})
    assert "64_group" in group(T.G_ILV) and "64_group" in group(T.G_ILV, {"wgrad_ilv": 1})
    for ilv in (0, 1):
        assert "big64" in single("bf16", T.G_ILV[0], {"wgrad_ilv": ilv, "wgrad_big_min": 1, "wgrad_big_slots": 8})
    # test_wgrad_group_equals_single_launches (its operands: a bias gradient where Cout >= 64 and the stride is 1)
    probs = [T.prob("bf16", s, "scale+db+ws" if s[4] >= 64 and s[6] == 1 else "scale+ws") for s in T.G_SINGLES]
    for knobs in ({}, {"wgrad_big_group": 0}, {"wgrad_ordered": 0}, {"wgrad_big_group": 0, "wgrad_ordered": 0}):
        name = group(probs, knobs)
        ordered = " ordered" if knobs.get("wgrad_ordered", 1) else ""
        if knobs.get("wgrad_big_group", 1):
            assert name.startswith("wgrad_bf16_lean64_group n=1") and "| wgrad_bf16_big64_group n=7" in name and name.endswith(ordered or name[-1]), name
            assert 128 <= int(name.split("wgrad_bf16_big64_group")[1].split("wgs=")[1].split()[0]) <= 1024, name
        else:
            assert name.startswith("wgrad_bf16_lean64_group n=7") and (ordered in name), name
            assert 300 <= int(name.split("wgs=")[1].split()[0]) <= 2400, name
    # the issue's two examples of the strings' shape
    assert re.fullmatch(r"wgrad_bf16_lean splits=\d+ ordered", single("bf16", (4, 50, 84, 256, 256, 3, 1, 1)))
    assert re.fullmatch(r"wgrad_bf16_lean64_group n=1 wgs=\d+ pix=\d+ ordered \| wgrad_bf16_big64_group n=7 wgs=\d+ pix=\d+ ordered", group(probs))
    # the threshold knobs: the three recorded values (at, above, below the problems' own count) straddle the rule
    for shapes, knob, count, beside in T.THRESHOLDS:
        names = []
        for v in (count - 1, count, count + 1):
            kn = dict(beside, **{knob: v})
            names.append(single("bf16", shapes[0], kn) if _key(["s", T.prob("bf16", shapes[0])], kn) in by_key else group(shapes, kn))
        assert len(set(names)) == 2, (knob, names)


def test_every_launch_form_is_reached_by_a_recorded_row(table):
    """the form list (WGRAD_FORMS, csrc/wgrad_select.h) against the names in the table; the ilv modifier by its knob on each template that has it"""
    src = open(os.path.join(ROOT, "aldi_amd", "csrc", "wgrad_select.h")).read()
    forms = re.findall(r'X\((WG_\w+),\s*"(\w+)",\s*\d+,\s*\d+\)', src)
    assert len(forms) == src[src.index("#define WGRAD_FORMS(X)"):src.index("enum WgForm")].count(" X(") == 12 and len({f[0] for f in forms}) == 12
    kernels = set()
    for _, knobs, name, _ in table:
        for part in name.split(" | "):
            kernels.add((part.split(" ")[0], bool(knobs.get("wgrad_ilv"))))
    for fid, printed in forms:
        want = printed + "_db" if fid == "WG_LEAN_GROUP_DB" else printed
        assert (want, False) in kernels, fid
    for printed in ("wgrad_bf16_big64", "wgrad_bf16_big64_group", "wgrad_bf16_lean64_group"):
        assert (printed, True) in kernels, printed


def test_plan_reports_argument_errors_like_the_launch():
    """every one of these returns before any HIP call (there is no GPU here): status and text of the launch == of the plan"""
    from aldi_amd import _lib as L
    T = _tool()
    buf = C.create_string_buffer(64)
    ok = T.prob("bf16", (2, 25, 42, 256, 256, 3, 1, 1), "scale+db+ws")

    def one(p, ws_bytes=BIG_WS, **over):
        arr = _args(L, T, ["s", p], {}, ws_bytes)
        for k, v in over.items():
            setattr(arr[0], k, v)
        return arr

    bad = [(L.WgradArgs * 1)(),                                                             # all null
           one(ok, dw=None),
           one(T.prob("bf16", (2, 8, 8, 20, 64, 1, 1, 0))),                                 # Cin: not a 16-byte multiple
           one(T.prob("f32", (2, 8, 8, 64, 66, 1, 1, 0), "scale")),                         # Cout
           one(T.prob("bf16", (1 << 11, 1 << 10, 1 << 10, 8, 8, 1, 1, 0))),                 # M = 2^31
           one(ok, Ho=0),
           one(T.prob("bf16", (64, 512, 512, 64, 8, 1, 1, 0))),                             # x: 2 GiB
           one(T.prob("bf16", (1, 4, 4, 32768, 16384, 1, 1, 0))),                           # dw: 2 GiB
           one(ok, dtype=7),
           one(ok, ws_bytes=1024)]                                                          # 2100 pixels in 7 ranges: the ordered epilogue needs more
    texts = set()
    for arr in bad:
        for group in (0, 1):
            rc_run = L.lib.aldi_conv_wgrad_group(arr, 1, None) if group else L.lib.aldi_conv_wgrad(arr, None)
            msg_run = L.lib.aldi_last_error()
            rc_plan = L.lib.aldi_conv_wgrad_plan(arr, 1, group, buf, len(buf), None)
            assert rc_run == rc_plan == -2 and L.lib.aldi_last_error() == msg_run and msg_run.startswith(b"conv_wgrad"), (group, msg_run)
            texts.add(msg_run)
    assert texts == {b"conv_wgrad: null pointer", b"conv_wgrad: Cin/Cout must be multiples of a 16-B chunk", b"conv_wgrad: bad M",
                     b"conv_wgrad: operand larger than 2 GiB (32-bit buffer offsets)", b"conv_wgrad: gradient larger than 2 GiB (32-bit buffer offsets)",
                     b"conv_wgrad: bad dtype", b"conv_wgrad: workspace too small (aldi_conv_wgrad_group_workspace)",
                     b"conv_wgrad_group: workspace too small (aldi_conv_wgrad_group_workspace)"}
    assert L.lib.aldi_conv_wgrad_group_workspace(bad[2], 1) == -1
    # n < 1, no array
    arr = one(ok)
    for n, a in ((0, arr), (-3, arr), (1, None)):
        rc_run = L.lib.aldi_conv_wgrad_group(a, n, None)
        msg_run = L.lib.aldi_last_error()
        assert rc_run == L.lib.aldi_conv_wgrad_plan(a, n, 1, buf, len(buf), None) == -2 and L.lib.aldi_last_error() == msg_run == b"conv_wgrad_group: no problems"
    assert L.lib.aldi_conv_wgrad(None, None) == L.lib.aldi_conv_wgrad_plan(None, 1, 0, buf, len(buf), None) == -2 and L.lib.aldi_last_error() == b"conv_wgrad: null pointer"
    # a bad problem behind good ones, and a workspace that the group outgrows: nothing is planned past the error, the text is the launch's
    three = _args(L, T, ["g", ok, T.prob("bf16", (2, 25, 42, 64, 96, 3, 1, 1)), T.prob("bf16", (2, 8, 8, 20, 64, 1, 1, 0))], {})
    small = _args(L, T, ["g"] + [T.prob("bf16", (4, 50, 84, 256, 256, 3, 1, 1), "ws")] * 3, {"wgrad_big_group": 0, "wgrad_group_slots": 4000}, 4096)
    for arr, text in ((three, b"conv_wgrad: Cin/Cout must be multiples of a 16-B chunk"), (small, b"conv_wgrad_group: workspace too small (aldi_conv_wgrad_group_workspace)")):
        rc_run = L.lib.aldi_conv_wgrad_group(arr, 3, None)
        msg_run = L.lib.aldi_last_error()
        assert rc_run == L.lib.aldi_conv_wgrad_plan(arr, 3, 1, buf, len(buf), None) == -2 and L.lib.aldi_last_error() == msg_run == text
    with pytest.raises(L.AldiHipError):
        L.plan_wgrad_dispatch(bad[0])


def test_plan_leaves_last_dispatch_alone_and_respects_the_buffer():
    from aldi_amd import _lib as L
    T = _tool()
    arr = _args(L, T, ["s", T.prob("bf16", (2, 25, 42, 256, 256, 3, 1, 1))], {})
    before = L.last_dispatch()
    need = 36 * 7 * 128 * 128 * 4          # 2 x 18 tiles of 128 x 128; 33 slabs of 64 pixels, at least 4 behind an epilogue: 5 each, 7 ranges
    query = L.lib.aldi_conv_wgrad_group_workspace(arr, 1)          # (n = 1: the larger of this launch's and the one-problem group's)
    assert query >= need
    assert L.plan_wgrad_dispatch(arr) == ("wgrad_bf16_lean splits=7 ordered", query) and L.last_dispatch() == before
    arr[0].ws = None
    assert L.plan_wgrad_dispatch(arr) == ("wgrad_bf16_lean splits=7", query)          # atomic epilogue; the query still answers for the ordered one
    buf = C.create_string_buffer(b"x" * 16, 16)
    ws = C.c_long(-5)
    assert L.lib.aldi_conv_wgrad_plan(arr, 1, 0, buf, 8, C.byref(ws)) == 0 and buf.raw == b"wgrad_b\0" + b"x" * 8 and ws.value == query
    assert L.lib.aldi_conv_wgrad_plan(arr, 1, 1, None, 0, None) == 0 and L.last_dispatch() == before

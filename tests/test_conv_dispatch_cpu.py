"""Which kernel a convolution gets, checked without a GPU: aldi_conv_igemm_plan (the dry run of aldi_conv_igemm / aldi_conv_igemm_group:
csrc/igemm_select.h) against tests/golden/conv_dispatch_table.json, which tools/record_conv_dispatch.py recorded from real launches
(aldi_last_dispatch() after each) BEFORE the selection was separated from the launch.  A threshold or rule edit shows here as the rows it moves."""
import ctypes as C
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_table.json")
DUMMY = 0x10000          # a non-null address: the plan never dereferences it


def _tool():
    spec = importlib.util.spec_from_file_location("record_conv_dispatch", os.path.join(ROOT, "tools", "record_conv_dispatch.py"))
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


def _plan(L, T, case, knobs):
    L.reset_tuning()
    for k, v in knobs.items():
        L.set_tuning(k, v)
    ptr = {f: DUMMY for f in T.PTR_FIELDS}
    if case[0] == "s":
        return L.plan_dispatch(T.conv_args(L, case[1], ptr))
    arr = (L.ConvArgs * (len(case) - 1))(*[T.conv_args(L, p, ptr) for p in case[1:]])
    return L.plan_dispatch(arr, len(case) - 1)


def test_plan_reproduces_every_recorded_row(table):
    from aldi_amd import _lib as L
    T = _tool()
    bad = [(case, knobs, name, got) for case, knobs, name in table for got in [_plan(L, T, case, knobs)] if got != name]
    assert not bad, (len(bad), bad[:5])


def _key(case, knobs):
    return json.dumps([case, knobs], sort_keys=True)


def test_recorded_rows_agree_with_the_names_the_gpu_tests_assert(table):
    """a bad recording cannot go unnoticed: rows looked up by (shape, operands, knobs) against the literal strings of tests/test_dispatch_gpu.py"""
    T = _tool()
    by_key = {_key(case, knobs): name for case, knobs, name in table}

    def single(dt, shape, ops, knobs=None, **kw):
        return by_key[_key(["s", T.prob(dt, shape, ops, **kw)], knobs or {})]

    full_fwd = [        # FULL_FWD (staged epilogue: _check_forward turns igemm_direct off)
        ((4, 200, 336, 256, 256, 3, 1, 1), "igemm<bf16,256,256,4,2,halo64>"), ((2, 200, 336, 256, 256, 3, 1, 1), "igemm<bf16,256,256,4,2,halo64>"),
        ((4, 100, 168, 256, 256, 3, 1, 1), "igemm<bf16,256,256,4,2,halo64>"), ((2, 100, 168, 256, 256, 3, 1, 1), "igemm<bf16,128,64,4,1,flat,halo>"),
        ((4, 50, 84, 256, 256, 3, 1, 1), "igemm<bf16,128,64,4,1,flat,halo>"), ((4, 200, 336, 64, 64, 3, 1, 1), "igemm<bf16,128,64,4,1,flat,halo>"),
        ((4, 200, 336, 64, 256, 1, 1, 0), "igemm<bf16,128,64,4,1,pipe,tap>"), ((4, 200, 336, 256, 64, 1, 1, 0), "igemm<bf16,128,64,4,1,pipe,tap>"),
        ((4, 200, 336, 256, 512, 1, 2, 0), "igemm<bf16,128,64,4,1,pipe,tap>"), ((4, 50, 84, 768, 1024, 1, 2, 0), "igemm<bf16,128,128,2,2,pipe,tap>"),
        ((4, 200, 336, 256, 16, 1, 1, 0), "igemm<bf16,128,16,4,1,pipe,tap>"), ((1, 120, 140, 3072, 768, 1, 1, 0), "igemm<bf16,256,128,4,2,flat,tap,k64>"),
        ((2048, 1, 1, 12544, 1024, 1, 1, 0), "igemm<bf16,64,64,2,2,flat,tap,k64>"), ((4, 25, 42, 512, 2048, 1, 1, 0), "igemm<bf16,128,64,4,1,pipe,tap>"),
        ((2, 25, 42, 512, 512, 3, 1, 1), "igemm<bf16,128,64,4,1,flat,halo>")]
    for shape, expect in full_fwd:
        assert single("bf16", shape, "y+scale+shift+relu+res1", {"igemm_direct": 0}) == expect, shape
    # fp32 parity mode (test_forward_default_dispatch_fullsize_fp32)
    assert single("f32", (2, 200, 336, 256, 256, 3, 1, 1), "y+scale+shift+relu+res1") == "igemm<f32,64,64,2,2,pipe,tap>"
    assert single("f32", (2, 200, 336, 256, 256, 3, 1, 1), "y+scale+shift+relu", {"igemm_f32_tile64_max": 0}) == "igemm<f32,256,128,4,2,flat,tap>"
    assert single("f32", (2, 200, 336, 64, 256, 1, 1, 0), "y+scale+shift+relu", {"igemm_f32_tile64_max": 0}) == "igemm<f32,128,128,2,2,pipe,tap>"
    assert single("f32", (2, 200, 336, 256, 256, 3, 1, 1), "y+scale+shift+relu", {"igemm_halo_f32": 400}) == "igemm<f32,256,128,4,2,flat,halo>"
    assert single("f32", (2, 100, 168, 128, 128, 3, 1, 1), "y+scale+shift+relu", {"igemm_halo_f32": 400}) == "igemm<f32,128,64,4,1,flat,halo>"
    assert single("f32", (2, 25, 42, 512, 512, 3, 1, 1), "y+scale+shift+relu", {"igemm_halo_f32": 400}) == "igemm<f32,64,64,2,2,pipe,tap>"
    # the direct epilogue and the weight-stationary kernel (DIRECT_FULL)
    assert single("bf16", (4, 50, 84, 256, 1024, 1, 1, 0), "y+scale+shift+relu+res1") == "igemm<bf16,128,64,4,1,pipe,tap,direct+res>"
    assert single("bf16", (4, 100, 168, 128, 512, 1, 1, 0), "y+scale+shift+relu+res1") == "igemm_ws<bf16,32,256,k128>"
    assert single("bf16", (4, 100, 168, 512, 128, 1, 1, 0), "y+mbits") == "igemm_ws<bf16,16,128,k512>"
    assert single("bf16", (4, 50, 84, 1024, 256, 1, 1, 0), "y+mbits") == "igemm<bf16,64,64,2,2,flat,tap,k64,direct>"
    assert single("bf16", (4, 100, 168, 512, 256, 1, 1, 0), "y+shift+res2") == "igemm<bf16,128,64,4,1,pipe,tap,direct+res>"
    assert single("bf16", (4, 200, 336, 256, 256, 3, 1, 1), "y") == "igemm<bf16,256,256,4,2,halo64,direct>"
    # test_weight_stationary_kernel_eligibility
    assert not single("bf16", (2, 100, 168, 128, 512, 1, 1, 0), "y").startswith("igemm_ws")                              # 33 600 pixels < igemm_ws_min
    assert not single("bf16", (1, 40, 50, 128, 512, 1, 1, 0), "y", {"igemm_ws_min": 4096}).startswith("igemm_ws")
    assert not single("bf16", (2, 50, 84, 512, 256, 1, 1, 0), "y+res2", {"igemm_ws_min": 4096}).startswith("igemm_ws")
    assert single("bf16", (2, 100, 168, 256, 256, 1, 1, 0), "y+res2", {"igemm_ws_min": 4096}) == "igemm_ws<bf16,32,128,k256>"
    assert not single("bf16", (2, 50, 84, 512, 256, 1, 1, 0), "y32").startswith("igemm_ws")
    assert not single("bf16", (2, 50, 84, 1024, 256, 1, 1, 0), "y", {"igemm_ws_min": 4096}).startswith("igemm_ws")
    assert not single("bf16", (2, 50, 84, 128, 384, 1, 1, 0), "y", {"igemm_ws_min": 4096}).startswith("igemm_ws")
    assert single("bf16", (2, 50, 84, 128, 512, 1, 1, 0), "y", {"igemm_ws_min": 4096}) == "igemm_ws<bf16,32,256,k128>"
    # the halo64_mid / halo_small / halo96 knob tests
    assert single("bf16", (4, 50, 84, 256, 256, 3, 1, 1), "y+relu") == "igemm<bf16,128,64,4,1,flat,halo,direct>"
    assert single("bf16", (4, 50, 84, 256, 256, 3, 1, 1), "y+relu", {"igemm_halo64_mid": 256}) == "igemm<bf16,128,128,2,2,halo64,direct>"
    assert single("bf16", (2, 25, 42, 512, 512, 3, 1, 1), "y+relu") == "igemm<bf16,128,64,4,1,flat,halo,direct>"
    assert single("bf16", (2, 25, 42, 512, 512, 3, 1, 1), "y+relu", {"igemm_halo_small": 320}) == "igemm<bf16,64,64,2,2,flat,halo,direct>"
    assert single("bf16", (4, 50, 84, 256, 256, 3, 1, 1), "y+relu", {"igemm_halo96": 1}) == "igemm<bf16,96,64,3,1,flat,halo,direct>"
    # the threshold knobs: the three recorded values (at, above, below the shape's own count) straddle the rule
    for shape, dt, ops, knob, count in (((4, 100, 168, 256, 256, 3, 1, 1), "bf16", "y+scale+shift+relu", "igemm_bigtile_min", 1050),
                                        ((1, 120, 140, 3072, 768, 1, 1, 0), "bf16", "y+scale+shift+relu", "igemm_lintile_min", 792),
                                        ((1, 120, 140, 3072, 768, 1, 1, 0), "bf16", "y+scale+shift+relu", "igemm_bigtile_k", 3072),
                                        ((4, 50, 84, 1024, 256, 1, 1, 0), "bf16", "y+scale+shift+relu", "igemm_k64_min", 1024),
                                        ((4, 25, 42, 512, 2048, 1, 1, 0), "bf16", "y+scale+shift+relu", "igemm_narrow_k", 512),
                                        ((4, 100, 168, 128, 512, 1, 1, 0), "bf16", "y+scale+shift+relu", "igemm_ws_min", 67200),
                                        ((2, 100, 168, 128, 128, 3, 1, 1), "f32", "y", "igemm_f32_tile64_max", 264),
                                        ((2, 100, 168, 128, 128, 3, 1, 1), "f32", "y", "igemm_halo_f32", 526)):
        names = [single(dt, shape, ops, {knob: v}) for v in (count - 1, count, count + 1)]
        assert len(set(names)) == 2, (knob, names)
    # split-K (test_splitk_linear_equals_plain)
    assert single("bf16", (2048, 1, 1, 12544, 1024, 1, 1, 0), "y+scale+shift+relu", ksplit=4) == "igemm<bf16,256,128,4,2,flat,tap,k64> splitk"
    assert single("bf16", (2048, 1, 1, 12544, 1024, 1, 1, 0), "y+scale+shift+relu", {"igemm_splitk_tile": 1}, ksplit=4) == "igemm<bf16,256,128,4,2,flat,tap> splitk"
    # groups (test_halo64_group_over_pyramid_levels, GROUP_CASES)
    pyr5 = ["g"] + [T.prob("bf16", (N, H, W, 256, 256, 3, 1, 1), "y+shift+relu") for (N, H, W) in ((2, 200, 336), (2, 100, 168), (2, 50, 84), (2, 25, 42), (2, 13, 21))]
    assert by_key[_key(pyr5, {})] == "igemm_group5<bf16,256,256,4,2,halo64,direct>"
    assert by_key[_key(pyr5, {"igemm_bigtile": 4})] == "igemm_group5<bf16,256,128,4,2,flat,halo>"
    pair = ["g"] + [T.prob("bf16", (N, 50, 84, 1024, 256, 1, 1, 0), "y+scale+shift+relu+res1") for N in (4, 2)]
    assert by_key[_key(pair, {})] == "igemm_group2<bf16,64,64,2,2,flat,tap,k64>"
    assert not by_key[_key(pair, {"igemm_group": 0})].startswith("igemm_group")


def test_every_tile_variant_is_reached_by_a_recorded_row(table):
    """the variant list (IGEMM_TILES, csrc/igemm_select.h) against the names in the table: every row of the list is some recorded row's kernel"""
    src = open(os.path.join(ROOT, "aldi_amd", "csrc", "igemm_select.h")).read()
    rows = re.findall(r"X\((\w+),\s*(bf16_t|float),\s*(TAP|HALO|ROLES|HALO64|WS),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d),\s*(\d)\)", src)
    assert len(rows) == src[src.index("#define IGEMM_TILES(X)"):src.index("enum TileForm")].count(" X(") and len({r[0] for r in rows}) == len(rows)
    names = {name.replace("_group", "G") for _, _, name in table}
    names = {re.sub(r"^igemmG\d+<", "igemm<", n).replace(" splitk", "").replace(",lockstep", "") for n in names}
    missing = []
    for tid, elem, form, BM, BN, WM, WN, KC, pipe, epi in rows:
        e = "f32" if elem == "float" else "bf16"
        if form == "WS":
            want = ["igemm_ws<%s,%s,%s,k%d>" % (e, BM, BN, int(KC) * 8)]
        elif form == "HALO64":
            want = ["igemm<%s,%s,%s,%s,%s,halo64%s>" % (e, BM, BN, WM, WN, d) for d in ("", ",direct")]
        elif form == "ROLES":
            want = ["igemm<%s,%s,%s,%s,%s,roles,halo>" % (e, BM, BN, WM, WN)]
        else:
            want = ["igemm<%s,%s,%s,%s,%s,%s,%s%s%s>" % (e, BM, BN, WM, WN, "pipe" if pipe == "1" else "flat", "halo" if form == "HALO" else "tap",
                                                       ",k64" if KC == "8" else "", {"0": "", "1": ",direct", "2": ",direct+res"}[epi])]
        if not any(w in names for w in want):
            missing.append(tid)
    assert not missing, missing


def test_plan_reports_argument_errors_like_the_launch():
    from aldi_amd import _lib as L
    T = _tool()
    ptr = {f: DUMMY for f in T.PTR_FIELDS}
    buf = C.create_string_buffer(64)
    bad = [L.ConvArgs(),                                                                        # all null
           T.conv_args(L, T.prob("bf16", (2, 8, 8, 20, 64, 3, 1, 1), "y"), ptr),                # Cin of a 3x3 conv
           T.conv_args(L, T.prob("bf16", (2, 8, 8, 64, 66, 1, 1, 0), "y"), ptr),                # Cout % 4
           T.conv_args(L, T.prob("bf16", (2, 7, 8, 64, 64, 1, 1, 0), "y+res2"), ptr),           # upsampled residual on an odd map
           T.conv_args(L, T.prob("f32", (2, 8, 8, 64, 64, 1, 1, 0), "y+mbits"), ptr),           # mask bits in fp32
           T.conv_args(L, T.prob("bf16", (2, 8, 8, 96, 64, 1, 1, 0), "y", ksplit=4), dict(ptr, ws=DUMMY))]      # split-K: K % 256
    for a in bad:
        rc_run = L.lib.aldi_conv_igemm(C.byref(a), None)
        msg_run = L.lib.aldi_last_error()
        rc_plan = L.lib.aldi_conv_igemm_plan(C.byref(a), 1, buf, len(buf))
        assert rc_run == rc_plan == -2 and L.lib.aldi_last_error() == msg_run and msg_run.startswith(b"conv_igemm:")
    arr = (L.ConvArgs * 2)(T.conv_args(L, T.prob("bf16", (2, 8, 8, 64, 64, 1, 1, 0), "y"), ptr), bad[2])
    rc_run = L.lib.aldi_conv_igemm_group(arr, 0, None)
    msg_run = L.lib.aldi_last_error()
    assert rc_run == L.lib.aldi_conv_igemm_plan(arr, 0, buf, len(buf)) == -2 and L.lib.aldi_last_error() == msg_run == b"conv_igemm_group: no problems"
    assert L.lib.aldi_conv_igemm_plan(arr, 2, buf, len(buf)) == -2 and b"Cout" in L.lib.aldi_last_error()      # different layers: single plans, the second fails
    arr[0].Cout = 66                                                                             # one layer shape: the group's own checks
    rc_run = L.lib.aldi_conv_igemm_group(arr, 2, None)
    msg_run = L.lib.aldi_last_error()
    assert rc_run == L.lib.aldi_conv_igemm_plan(arr, 2, buf, len(buf)) == -2 and L.lib.aldi_last_error() == msg_run and b"Cout" in msg_run
    with pytest.raises(L.AldiHipError):
        L.plan_dispatch(bad[0])


def test_plan_leaves_last_dispatch_alone_and_respects_the_buffer():
    from aldi_amd import _lib as L
    T = _tool()
    a = T.conv_args(L, T.prob("bf16", (2, 25, 42, 64, 96, 3, 1, 1), "y"), {f: DUMMY for f in T.PTR_FIELDS})
    before = L.last_dispatch()
    assert L.plan_dispatch(a) == "igemm<bf16,128,64,4,1,flat,halo,direct>" and L.last_dispatch() == before
    buf = C.create_string_buffer(b"x" * 16, 16)
    assert L.lib.aldi_conv_igemm_plan(C.byref(a), 1, buf, 8) == 0 and buf.raw == b"igemm<b\0" + b"x" * 8
    assert L.lib.aldi_conv_igemm_plan(C.byref(a), 1, None, 0) == 0


def test_every_documented_knob_exists_and_every_knob_is_documented():
    """the knob list (ALDI_KNOBS, csrc/host.h -> AldiTuning and aldi_set/get_tuning's table) against the comment of include/aldi_hip.h"""
    from aldi_amd import _lib as L
    src = open(L.HEADER_PATH).read()
    doc = src[src.index("Tuning knobs of the kernel dispatchers"):src.index("int aldi_set_tuning")]
    documented = set()
    for line in doc.splitlines():
        m = re.match(r"\s*\*   ([a-z0-9_]+(?:, [a-z0-9_]+)*) ", line)
        if m:
            documented.update(m.group(1).split(", "))
    listed = set(re.findall(r"X\((\w+), -?\d+\)", open(os.path.join(ROOT, "aldi_amd", "csrc", "host.h")).read()))
    assert len(listed) >= 60
    v = C.c_int(0)
    for name in sorted(documented | listed):
        assert L.lib.aldi_get_tuning(name.encode(), C.byref(v)) == 0, name
    assert documented == listed, documented ^ listed
    assert L.lib.aldi_get_tuning(b"no_such_knob", C.byref(v)) == -2

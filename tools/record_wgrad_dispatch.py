"""Record which kernels aldi_conv_wgrad / aldi_conv_wgrad_group launch, and the workspace their ordered epilogue asks for, over a sweep of
(shapes, operands, knobs): the table behind tests/test_wgrad_dispatch_cpu.py (tests/golden/wgrad_dispatch_table.json).

    python tools/record_wgrad_dispatch.py --out tests/golden/wgrad_dispatch_table.json [--time-limit 600]

Needs a GPU: every row is a real launch on buffers allocated once at the sweep's largest sizes, and the name is what aldi_last_dispatch()
reports after it; ws_bytes is what aldi_conv_wgrad_group_workspace answers for the same arguments.  Uses aldi_conv_wgrad,
aldi_conv_wgrad_group, aldi_conv_wgrad_group_workspace, aldi_set_tuning and aldi_last_dispatch only.  Stops at the first non-zero status
(or past the time limit) with a non-zero exit code and launches nothing more.  No value is read back: names and bytes only.

Row: [case, knobs, name, ws_bytes];  case = ["s", prob] (aldi_conv_wgrad) or ["g", prob, prob, ...] (aldi_conv_wgrad_group);
prob = [dtype, N, H, W, Cin, Cout, k, stride, pad, flags];  flags = '+'-joined names out of scale, db, ws (the call gets a workspace: read
from the first problem) and dw<i> (the problem adds into gradient buffer i -- and bias buffer i -- instead of its own: how two problems
share one);  knobs = {name: value} on top of the defaults.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _conv_tool():
    spec = importlib.util.spec_from_file_location("record_conv_dispatch", os.path.join(ROOT, "tools", "record_conv_dispatch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CT = _conv_tool()
_uniq = CT._uniq

# ---------------------------------------------------------------------------------- shapes: (N, H, W, Cin, Cout, k, stride, pad)
# tests/test_dispatch_gpu.py's weight-gradient tables
FULL_BF16 = [(4, 200, 336, 256, 256, 3, 1, 1), (4, 100, 168, 256, 256, 3, 1, 1), (4, 200, 336, 256, 256, 1, 1, 0), (4, 50, 84, 256, 256, 3, 1, 1),
             (4, 50, 84, 1024, 256, 1, 1, 0), (4, 100, 168, 128, 512, 1, 1, 0), (4, 200, 336, 256, 512, 1, 2, 0), (2048, 1, 1, 12544, 1024, 1, 1, 0),
             (4, 200, 336, 256, 16, 1, 1, 0), (2, 200, 336, 256, 256, 3, 1, 0)]
SMALL = [(2, 25, 42, 256, 256, 3, 1, 1), (1, 19, 23, 256, 512, 1, 1, 0), (3, 9, 130, 64, 256, 3, 1, 1)]
SPLIT_CASE = (2, 50, 84, 256, 256, 3, 1, 1)
BIG_ARM = [(4, 100, 168, 256, 256, 3, 1, 1), (2, 25, 42, 256, 256, 3, 1, 1), (1, 19, 23, 256, 512, 1, 1, 0), (2048, 1, 1, 1024, 256, 1, 1, 0)]
F32_CASES = [(2, 100, 168, 256, 256, 3, 1, 1), (44646, 1, 1, 256, 1024, 1, 1, 0), (44646, 1, 1, 1024, 256, 1, 1, 0), (600, 1, 1, 256, 92, 1, 1, 0),
             (2, 50, 84, 1024, 256, 1, 2, 0), (2, 23, 37, 132, 200, 3, 1, 1), (2, 200, 336, 64, 64, 3, 1, 1)]
DMA_CASES = [(2, 25, 42, 256, 256, 3, 1, 1), (1, 19, 23, 256, 512, 1, 1, 0), (3, 9, 130, 64, 256, 3, 1, 1), (2, 13, 21, 256, 256, 3, 1, 1),
             (4, 1, 1, 1032, 48, 1, 1, 0), (4, 50, 84, 256, 256, 3, 1, 1), (4, 100, 168, 128, 512, 1, 1, 0), (4, 200, 336, 256, 256, 3, 1, 1),
             (2048, 1, 1, 12544, 1024, 1, 1, 0), (4, 200, 336, 256, 16, 1, 1, 0)]
BIAS_CASES = [(2, 50, 84, 256, 512, 1, 1, 0), (2, 25, 42, 128, 128, 3, 1, 1), (2, 200, 336, 256, 256, 3, 1, 1), (2, 50, 84, 256, 512, 1, 2, 0)]
# the groups of the tests: register-staged loops / interleaved loop; == single launches; ordered epilogue; shared buffers; split policy
G_LOOPS = [(4, 50, 84, 256, 256, 3, 1, 1), (4, 50, 84, 1024, 256, 1, 1, 0), (2, 100, 168, 128, 128, 3, 1, 1), (2, 100, 168, 512, 128, 1, 1, 0), (1, 37, 41, 72, 136, 1, 1, 0)]
G_ILV = G_LOOPS[:4] + [(2, 13, 21, 256, 256, 3, 1, 1)]
G_SINGLES = [(4, 50, 84, 256, 256, 3, 1, 1), (4, 50, 84, 1024, 256, 1, 1, 0), (4, 50, 84, 256, 1024, 1, 1, 0), (4, 50, 84, 256, 256, 3, 1, 1),
             (4, 25, 42, 512, 512, 3, 1, 1), (2, 200, 336, 256, 256, 3, 1, 1), (4, 100, 168, 256, 512, 1, 2, 0), (4096, 1, 1, 2304, 256, 1, 1, 0),
             (4096, 1, 1, 256, 16, 1, 1, 0)]
G_ORDERED = [(4, 50, 84, 256, 256, 3, 1, 1), (4, 50, 84, 1024, 256, 1, 1, 0), (2, 100, 168, 128, 128, 3, 1, 1), (4, 25, 42, 2048, 512, 1, 1, 0), (300, 1, 1, 1024, 1024, 1, 1, 0)]
G_POLICY = [(2, 25, 42, 256, 256, 3, 1, 1), (1, 19, 23, 256, 512, 1, 1, 0), (3, 9, 130, 64, 256, 3, 1, 1)]
G_LEAN = [(4, 100, 168, 128, 128, 3, 1, 1), (4, 100, 168, 512, 128, 1, 1, 0), (4, 100, 168, 128, 512, 1, 1, 0)]      # a res3 block: no 256-tile member
HAZARD = (4, 64, 64, 256, 256, 1, 1, 0)            # more than 24 of these: tests/test_dispatch_gpu.py's finalize-order test


def stage_groups(N):
    """what the engine collects per backward stage: the layers of res2..res5, the FPN / RPN convs, the box head (R50-FPN, 800 x 1344)"""
    out = []
    H, W, cin = 200, 336, 64
    for stage, (mid, cout, blocks) in enumerate([(64, 256, 3), (128, 512, 4), (256, 1024, 6), (512, 2048, 3)]):
        s = 1 if stage == 0 else 2
        Ho, Wo = H // s, W // s
        g = [(N, H, W, cin, mid, 1, s, 0), (N, H, W, cin, cout, 1, s, 0), (N, Ho, Wo, mid, mid, 3, 1, 1), (N, Ho, Wo, mid, cout, 1, 1, 0)]
        for _ in range(blocks - 1):
            g += [(N, Ho, Wo, cout, mid, 1, 1, 0), (N, Ho, Wo, mid, mid, 3, 1, 1), (N, Ho, Wo, mid, cout, 1, 1, 0)]
        out.append(g)
        H, W, cin = Ho, Wo, cout
    out.append([(N, 200 >> l, 336 >> l, c, 256, 1, 1, 0) for l, c in enumerate((256, 512, 1024, 2048))] + [(N, 200 >> l, 336 >> l, 256, 256, 3, 1, 1) for l in range(4)])
    R = 512 * N
    out.append([(R, 1, 1, 12544, 1024, 1, 1, 0), (R, 1, 1, 1024, 1024, 1, 1, 0), (R, 1, 1, 1024, 48, 1, 1, 0), (R, 1, 1, 1024, 16, 1, 1, 0)])
    return out


# ---------------------------------------------------------------------------------- problems
def out_hw(p):
    _, N, H, W, Cin, Cout, k, stride, pad = p[:9]
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def legal(p):
    """the argument rules of aldi_conv_wgrad (fill_wgdev)"""
    dt, N, H, W, Cin, Cout, k, stride, pad, flags = p
    Ho, Wo = out_hw(p)
    ep, esz = (8, 2) if dt == "bf16" else (4, 4)
    if Cin % ep or Cout % ep or Ho < 1 or Wo < 1 or N * Ho * Wo >= 2 ** 31:
        return False
    return max(N * H * W * Cin * esz, N * Ho * Wo * Cout * esz, Cout * k * k * Cin * 4) < 2 ** 31


def prob(dt, shape, flags="scale+ws"):
    return [dt] + list(shape) + [flags]


def dw_index(p, i):
    """which gradient / bias buffer problem i of a call adds into"""
    for f in p[9].split("+"):
        if f.startswith("dw"):
            return int(f[2:])
    return i


def sizes(p):
    """bytes of x, g, dw, db a problem needs"""
    dt, N, H, W, Cin, Cout, k, stride, pad, flags = p
    Ho, Wo = out_hw(p)
    esz = 2 if dt == "bf16" else 4
    return {"x": N * H * W * Cin * esz, "g": N * Ho * Wo * Cout * esz, "dw": Cout * k * k * Cin * 4, "db": Cout * 4}


def layout(case):
    """-> ([dw offset of each problem], [db offset], dw bytes, db bytes): buffer i of a call starts where buffer i - 1 ends (256-byte units)"""
    ps = case[1:]
    need_dw, need_db = {}, {}
    for i, p in enumerate(ps):
        j, s = dw_index(p, i), sizes(p)
        need_dw[j] = max(need_dw.get(j, 0), s["dw"])
        need_db[j] = max(need_db.get(j, 0), s["db"])
    off_dw, off_db, a, b = {}, {}, 0, 0
    for j in sorted(need_dw):
        off_dw[j], off_db[j] = a, b
        a += (need_dw[j] + 255) // 256 * 256
        b += (need_db[j] + 255) // 256 * 256
    return [off_dw[dw_index(p, i)] for i, p in enumerate(ps)], [off_db[dw_index(p, i)] for i, p in enumerate(ps)], a, b


def wgrad_args(L, case, ptr, ws_bytes=0):
    """the aldi_wgrad_args array of a case; ptr: {x, g, dw, db, scale, ws: address}"""
    ps = case[1:]
    off_dw, off_db, _, _ = layout(case)
    arr = (L.WgradArgs * len(ps))()
    for i, p in enumerate(ps):
        dt, N, H, W, Cin, Cout, k, stride, pad, flags = p
        f = set(flags.split("+"))
        Ho, Wo = out_hw(p)
        arr[i] = L.WgradArgs(ptr["x"], ptr["g"], ptr["dw"] + off_dw[i], ptr["scale"] if "scale" in f else None, N, H, W, Cin, Cout, k, k, stride, pad, Ho, Wo,
                             L.BF16 if dt == "bf16" else L.F32, ptr["db"] + off_db[i] if "db" in f else None, None, 0)
    if "ws" in ps[0][9].split("+"):
        arr[0].ws, arr[0].ws_bytes = ptr["ws"], ws_bytes
    return arr


# ---------------------------------------------------------------------------------- the sweep
# threshold knobs: (problems, knob, the shape's own count, knobs beside it).  The count is where the rule flips for THESE problems:
#   wgrad_big_min       (4,100,168,256,256,3x3): 1050 slabs of 64 pixels over floor(256 slots / 9 tiles) = 28 workgroups per tile -> 37 slabs each
#   wgrad_big_slots     the same layer: floor(slots / 9) <= 37 keeps 1050 / that >= wgrad_big_min = 28: 9 * 37 + 8 = 341 is the last such value
#   wgrad_slots         (4,50,84,256,256,3x3), lean: 2 x 18 = 36 tiles of 128 x 128 -> cdiv(slots, 36) splits
#   wgrad_group_slots   two res3 layers at N = 2 (9 + 4 tiles, unsplit 13 workgroups): a target above 13 halves the pixel range
#   wgrad_big_group_min (4,50,84,256,256,3x3) alone: 9 tiles x 16800 pixels = 36.9 x 4096 tile-pixels -> from 37 on it folds into the 128-tile group
#   wgrad_group_epi     res4's 19 layers at N = 4 on 128 x 128 tiles (wgrad_big_group 0): the round model, rounds x (T / 32 + epi), gives up a pixel split from 34 on
#   wgrad_big_epi       G_SINGLES' seven 256-tile layers: the same model on rounds of wgrad_big_slots gives up a split from 15 on
#                       (both found by stepping the knob through aldi_conv_wgrad_group_workspace, whose answer moves with the split)
THRESHOLDS = [([(4, 100, 168, 256, 256, 3, 1, 1)], "wgrad_big_min", 37, {}),
              ([(4, 100, 168, 256, 256, 3, 1, 1)], "wgrad_big_slots", 341, {}),
              ([(4, 50, 84, 256, 256, 3, 1, 1)], "wgrad_slots", 36, {"wgrad_big_min": 0}),
              ([(2, 100, 168, 128, 128, 3, 1, 1), (2, 100, 168, 512, 128, 1, 1, 0)], "wgrad_group_slots", 13, {}),
              ([(4, 50, 84, 256, 256, 3, 1, 1)], "wgrad_big_group_min", 37, {}),
              (stage_groups(4)[2], "wgrad_group_epi", 34, {"wgrad_big_group": 0}),
              (G_SINGLES, "wgrad_big_epi", 15, {})]


def sweep():
    """-> [(case, knobs)]"""
    rows = []

    def single(p, knobs=None):
        if legal(p):
            rows.append((["s", p], dict(knobs or {})))

    def group(ps, knobs=None):
        if all(legal(p) for p in ps):
            rows.append((["g"] + ps, dict(knobs or {})))

    def bgroup(shapes, knobs=None, flags="scale+db+ws", dt="bf16"):
        group([prob(dt, s, flags) for s in shapes], knobs)

    r50 = {N: _uniq(CT.r50_fpn(N)) for N in (2, 4, 6)}
    tests_bf16 = _uniq(FULL_BF16 + SMALL + [SPLIT_CASE] + BIG_ARM + DMA_CASES + BIAS_CASES)
    # defaults: every layer with and without a workspace (ordered / atomic epilogue) and with the bias gradient
    for s in _uniq(tests_bf16 + r50[4] + r50[2] + r50[6] + CT.token_linears()):
        single(prob("bf16", s, "scale+ws"))
        if s in tests_bf16 + r50[4]:
            single(prob("bf16", s, "scale"))
            single(prob("bf16", s, "db+ws"))
    for s in _uniq(F32_CASES + SMALL + CT.detr_trunk() + CT.FULL_F32 + [(1, 25, 42, 64, 64, 3, 1, 1)]):
        single(prob("f32", s, "scale"))
        single(prob("f32", s, "db"))
        single(prob("f32", s, "scale+ws"))
        single(prob("f32", s, "scale"), {"wgrad_f32_tile128": 0})
    # each non-default arm, one at a time
    arms = [{"wgrad_lean": 0}, {"wgrad_dma": 1}, {"wgrad_dma": 2}, {"wgrad_dma64": 0}, {"wgrad_dma64": 1}, {"wgrad_dma64": 2}, {"wgrad_ilv": 1}, {"wgrad_ordered": 0},
            {"wgrad_big_min": 0}, {"wgrad_big_min": 1}]
    for s in _uniq(tests_bf16 + r50[4]):
        for kn in arms:
            single(prob("bf16", s, "scale+ws"), kn)
        single(prob("bf16", s, "db+ws"), {"wgrad_dma": 2})                         # the bias pass behind the LDS-DMA kernel
    for s in SMALL:
        single(prob("bf16", s), {"wgrad_big_min": 1, "wgrad_big_slots": 2})
        single(prob("bf16", s), {"wgrad_big_min": 1, "wgrad_big_slots": 2, "wgrad_ilv": 1})
    for slots in (1, 64, 1000):
        single(prob("bf16", SPLIT_CASE), {"wgrad_slots": slots, "wgrad_big_min": 0})
        single(prob("bf16", SPLIT_CASE), {"wgrad_big_slots": slots, "wgrad_big_min": 1})
        single(prob("bf16", SPLIT_CASE), {"wgrad_dma": 2, "wgrad_slots": slots})
        single(prob("bf16", SPLIT_CASE), {"wgrad_dma": 2, "wgrad_slots": slots, "wgrad_big_min": 1})      # the 256 tile's split re-derived for 128
    for s in BIG_ARM:
        for d64 in (0, 1, 2, 3):
            single(prob("bf16", s), {"wgrad_dma64": d64, "wgrad_big_min": 1, "wgrad_big_slots": 8})
            single(prob("bf16", s), {"wgrad_dma64": d64, "wgrad_big_min": 1, "wgrad_big_slots": 8, "wgrad_ilv": 1})
    for ilv in (0, 1):                                                              # the interleaved loop's test: the 256 tile alone
        single(prob("bf16", G_ILV[0]), {"wgrad_ilv": ilv, "wgrad_big_min": 1, "wgrad_big_slots": 8})
    # clamps: fewer 256-tile slots than tiles (floor 0 -> 1 split); fp32's 512 splits
    single(prob("bf16", (4, 100, 168, 256, 256, 3, 1, 1)), {"wgrad_big_slots": 8, "wgrad_big_min": 1})
    single(prob("bf16", (4, 100, 168, 256, 256, 3, 1, 1)), {"wgrad_big_slots": 0, "wgrad_big_min": 1})
    single(prob("bf16", (4, 200, 336, 64, 64, 1, 1, 0)), {"wgrad_slots": 4000})
    single(prob("f32", (8, 200, 336, 16, 16, 1, 1, 0), "scale"), {"wgrad_slots": 100000})
    single(prob("f32", (8, 200, 336, 16, 16, 1, 1, 0), "scale"), {"wgrad_slots": 100000, "wgrad_f32_tile128": 0})
    # threshold knobs: at, one above and one below the shape's own count
    for shapes, name, count, beside in THRESHOLDS:
        for v in (count, count + 1, count - 1):
            kn = dict(beside, **{name: v})
            if len(shapes) == 1 and not name.startswith(("wgrad_big_group", "wgrad_group", "wgrad_big_epi")):
                single(prob("bf16", shapes[0]), kn)
            else:
                bgroup(shapes, kn)
    # groups
    gk = [{}, {"wgrad_big_group": 0}, {"wgrad_ordered": 0}, {"wgrad_big_group": 0, "wgrad_ordered": 0}, {"wgrad_dma64": 0}, {"wgrad_dma64": 1}, {"wgrad_dma64": 2},
          {"wgrad_ilv": 1}, {"wgrad_db": 1}, {"wgrad_db": 1, "wgrad_dma64": 0}, {"wgrad_lean": 0}, {"wgrad_group_slots": 1}, {"wgrad_group_slots": 4000}, {"wgrad_big_min": 1},
          {"wgrad_big_group_min": 100000}]
    named = [G_LOOPS, G_ILV, G_SINGLES, G_ORDERED, G_POLICY, G_LEAN]
    for shapes in named:
        for kn in gk:
            bgroup(shapes, kn)
        bgroup(shapes, {}, "scale")                                                # no workspace: the atomic epilogue
        bgroup(shapes, {}, "scale+ws")
    for N in (2, 4, 6):
        for shapes in stage_groups(N):
            for kn in gk[:4] + gk[4:5] + gk[7:9] if N == 4 else gk[:1]:
                bgroup(shapes, kn)
            bgroup(shapes, {}, "scale")
    group([prob("bf16", G_SINGLES[i], "scale+db+ws" if G_SINGLES[i][4] >= 64 and G_SINGLES[i][6] == 1 else "scale+ws") for i in range(9)])      # the test's operands
    for kn in gk[1:4]:
        group([prob("bf16", G_SINGLES[i], "scale+db+ws" if G_SINGLES[i][4] >= 64 and G_SINGLES[i][6] == 1 else "scale+ws") for i in range(9)], kn)
    # eligible and forwarded problems in one call (fp32, strided, unpadded, ragged channels)
    for kn in ({}, {"wgrad_ordered": 0}, {"wgrad_big_group": 0}, {"wgrad_dma": 2}):
        group([prob("bf16", (2, 50, 84, 256, 256, 3, 1, 1), "scale+db+ws"), prob("f32", (2, 50, 84, 64, 64, 3, 1, 1), "scale+db"), prob("bf16", (2, 50, 84, 256, 512, 1, 2, 0), "db"),
               prob("bf16", (2, 50, 84, 256, 256, 3, 1, 0), "scale"), prob("bf16", (2, 50, 84, 1024, 256, 1, 1, 0), "db"), prob("bf16", (2, 37, 41, 72, 136, 1, 1, 0), "scale")], kn)
        group([prob("f32", s, "scale+ws") for s in F32_CASES[3:6]], kn)                  # nothing grouped: the last single's name survives
        group([prob("bf16", (2, 50, 84, 256, 512, 1, 2, 0), "scale+ws"), prob("bf16", (4, 200, 336, 256, 256, 3, 1, 1), "scale")], kn)
    # layers that share a gradient / bias buffer (one conv on several pyramid levels): those keep the atomic epilogue
    pyr = [(2, 100, 168), (2, 50, 84), (2, 25, 42), (2, 13, 21)]
    for kn in ({}, {"wgrad_big_group": 0}, {"wgrad_ordered": 0}, {"wgrad_big_min": 1}):
        group([prob("bf16", (N, H, W, 256, 256, 3, 1, 1), "db+ws+dw0") for (N, H, W) in pyr] + [prob("bf16", (2, 50, 84, 512, 256, 1, 1, 0), "ws")], kn)
        group([prob("bf16", (N, H, W, 256, 256, 3, 1, 1), "scale+ws+dw0") for (N, H, W) in pyr], kn)      # every member shared
        group([prob("bf16", (N, H, W, 256, 16, 1, 1, 0), "db+ws+dw1") for (N, H, W) in pyr] + [prob("bf16", (2, 200, 336, 256, 256, 3, 1, 1), "db+ws")], kn)
    # n == 1 (the workspace query answers for aldi_conv_wgrad as well)
    for s in _uniq(FULL_BF16 + SMALL + [SPLIT_CASE]):
        bgroup([s])
        bgroup([s], {"wgrad_big_group": 0})
        bgroup([s], {"wgrad_slots": 1000, "wgrad_big_min": 0})
    group([prob("f32", F32_CASES[0], "scale+ws")])
    # more groups than one launch takes (24): the rest goes through single launches
    small_lean = (2, 25, 42, 64, 96, 3, 1, 1)
    for kn in ({}, {"wgrad_ordered": 0}, {"wgrad_slots": 1000}):
        bgroup([small_lean] * 26, kn)
        bgroup([(2, 25, 42, 256, 256, 3, 1, 1)] * 13 + [small_lean] * 13, kn)            # 13 + 13: the 256 set stays, or folds while both fit one group
        bgroup([(2, 25, 42, 256, 256, 3, 1, 1)] * 12 + [small_lean] * 13, kn)
    for kn in ({"wgrad_big_min": 1}, {"wgrad_big_min": 1, "wgrad_big_slots": 64}, {}, {"wgrad_big_min": 1, "wgrad_ordered": 0}, {"wgrad_big_group": 0}):
        bgroup([HAZARD] * 26, kn, "ws")
        bgroup([HAZARD] * 30, kn, "db+ws")
    seen, out = set(), []
    for case, knobs in rows:
        key = json.dumps([case, knobs], sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append((case, knobs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="the table to write (not needed with --count)")
    ap.add_argument("--time-limit", type=float, default=600.0, help="seconds; past it the run stops with exit code 3")
    ap.add_argument("--count", action="store_true", help="print the number of rows of the sweep and exit (no GPU)")
    a = ap.parse_args()
    rows = sweep()
    if a.count:
        print(len(rows))
        return 0
    if not a.out:
        ap.error("--out is required")
    import torch
    from aldi_amd import _lib as L

    def tune(knobs):
        L.lib.aldi_reset_tuning()
        for k, v in knobs.items():
            if L.lib.aldi_set_tuning(k.encode(), int(v)):
                raise SystemExit("unknown knob " + k)

    # sizes first (no GPU work): the workspace query of every row under its knobs, and the largest operands
    need = {"x": 0, "g": 0, "dw": 0, "db": 0, "scale": 1 << 16, "ws": 256}
    dummy = {f: 0x10000 for f in need}
    ws_of = []
    for case, knobs in rows:
        tune(knobs)
        ws = L.lib.aldi_conv_wgrad_group_workspace(wgrad_args(L, case, dummy), len(case) - 1)
        if ws < 0:
            print("workspace query: %s at %s %s" % (L.lib.aldi_last_error().decode(), case, knobs), file=sys.stderr)
            return 1
        ws_of.append(ws)
        need["ws"] = max(need["ws"], ws)
        for p in case[1:]:
            s = sizes(p)
            need["x"], need["g"] = max(need["x"], s["x"]), max(need["g"], s["g"])
        _, _, dwb, dbb = layout(case)
        need["dw"], need["db"] = max(need["dw"], dwb), max(need["db"], dbb)
    bufs = {f: torch.zeros(max(b, 256), dtype=torch.uint8, device="cuda") for f, b in need.items()}
    ptr = {f: t.data_ptr() for f, t in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.time()
    table = []
    for (case, knobs), ws in zip(rows, ws_of):
        if time.time() - t0 > a.time_limit:
            print("time limit after %d of %d rows" % (len(table), len(rows)), file=sys.stderr)
            return 3
        tune(knobs)
        arr = wgrad_args(L, case, ptr, need["ws"])
        if case[0] == "s":
            rc = L.lib.aldi_conv_wgrad(arr, stream)
        else:
            rc = L.lib.aldi_conv_wgrad_group(arr, len(case) - 1, stream)
        if rc:
            print("status %d (%s) at %s %s" % (rc, L.lib.aldi_last_error().decode(), case, knobs), file=sys.stderr)
            return 1
        name = L.lib.aldi_last_dispatch().decode()
        torch.cuda.synchronize()            # a fault surfaces here, at the row that caused it: nothing more is launched
        table.append([case, knobs, name, ws])
    L.lib.aldi_reset_tuning()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in table) + "\n]\n")
    print("%d rows, %d distinct names, %.1f s" % (len(table), len({r[2] for r in table}), time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())

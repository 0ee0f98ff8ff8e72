"""Record which kernel aldi_conv_igemm / aldi_conv_igemm_group pick over a sweep of (shape, operands, knobs): the table behind
tests/test_conv_dispatch_cpu.py (tests/golden/conv_dispatch_table.json).

    python tools/record_conv_dispatch.py --out tests/golden/conv_dispatch_table.json [--time-limit 600]

Needs a GPU: every row is a real launch on buffers allocated once at the sweep's largest sizes, and the name is what
aldi_last_dispatch() reports after it.  Uses aldi_conv_igemm, aldi_conv_igemm_group, aldi_set_tuning and aldi_last_dispatch only.
Stops at the first non-zero status (or past the time limit) with a non-zero exit code and launches nothing more.

Row: [case, knobs, name];  case = ["s", prob] (aldi_conv_igemm) or ["g", prob, prob, ...] (aldi_conv_igemm_group);
prob = [dtype, N, H, W, Cin, Cout, k, stride, pad, operands, ksplit, out_scale];  operands = '+'-joined names out of
y y32 scale shift relu res1 res2 mask mbits bout;  knobs = {name: value} on top of the defaults.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# ---------------------------------------------------------------------------------- shapes: (N, H, W, Cin, Cout, k, stride, pad)
# tests/test_dispatch_gpu.py's tables
FULL_FWD = [(4, 200, 336, 256, 256, 3, 1, 1), (2, 200, 336, 256, 256, 3, 1, 1), (4, 100, 168, 256, 256, 3, 1, 1), (2, 100, 168, 256, 256, 3, 1, 1),
            (4, 50, 84, 256, 256, 3, 1, 1), (4, 200, 336, 64, 64, 3, 1, 1), (4, 200, 336, 64, 256, 1, 1, 0), (4, 200, 336, 256, 64, 1, 1, 0),
            (4, 200, 336, 256, 512, 1, 2, 0), (4, 50, 84, 768, 1024, 1, 2, 0), (4, 200, 336, 256, 16, 1, 1, 0), (1, 120, 140, 3072, 768, 1, 1, 0),
            (2048, 1, 1, 12544, 1024, 1, 1, 0), (4, 25, 42, 512, 2048, 1, 1, 0), (2, 25, 42, 512, 512, 3, 1, 1)]
FULL_F32 = [(2, 200, 336, 256, 256, 3, 1, 1), (2, 200, 336, 64, 256, 1, 1, 0), (2, 200, 336, 64, 64, 3, 1, 1), (2, 25, 42, 512, 512, 3, 1, 1),
            (2, 100, 168, 128, 128, 3, 1, 1)]
SMALL = [(2, 25, 42, 64, 96, 3, 1, 1), (1, 19, 23, 128, 256, 3, 1, 1), (3, 9, 130, 32, 64, 3, 1, 1), (2, 24, 40, 256, 72, 1, 1, 0),
         (2, 25, 41, 256, 136, 1, 2, 0), (2, 10, 12, 64, 68, 3, 1, 0), (1, 17, 19, 64, 16, 3, 2, 1), (5, 1, 1, 1032, 48, 1, 1, 0)]
K64 = [(2, 24, 40, 256, 72, 1, 1, 0), (5, 1, 1, 1032, 48, 1, 1, 0), (3, 7, 9, 64, 200, 1, 1, 0), (130, 1, 1, 2048, 136, 1, 1, 0), (130, 1, 1, 512, 136, 1, 1, 0)]
DGRAD = [(4, 200, 336, 256, 256, 3, 1, 1), (4, 50, 84, 256, 256, 3, 1, 1), (4, 50, 84, 1024, 256, 1, 1, 0), (2, 37, 53, 64, 128, 3, 1, 1)]
DIRECT_FULL = [(4, 50, 84, 256, 1024, 1, 1, 0), (4, 100, 168, 128, 512, 1, 1, 0), (2, 25, 42, 512, 2048, 1, 1, 0), (4, 50, 84, 1024, 256, 1, 1, 0),
               (4, 100, 168, 512, 128, 1, 1, 0), (4, 100, 168, 512, 1024, 1, 2, 0), (4, 100, 168, 512, 256, 1, 1, 0), (4, 25, 42, 2048, 256, 1, 1, 0)]
DIRECT_SMALL = [(2, 25, 42, 64, 96, 3, 1, 1), (1, 19, 23, 128, 256, 3, 1, 1), (2, 24, 40, 256, 72, 1, 1, 0), (2, 25, 41, 256, 136, 1, 2, 0),
                (3, 7, 9, 64, 200, 1, 1, 0), (1, 5, 6, 32, 64, 1, 1, 0), (130, 1, 1, 2048, 136, 1, 1, 0)]
WS_SMALL = [(3, 7, 9, 64, 256, 1, 1, 0), (2, 25, 41, 128, 512, 1, 1, 0), (1, 19, 23, 256, 256, 1, 1, 0), (2, 13, 30, 512, 128, 1, 1, 0),
            (130, 1, 1, 128, 768, 1, 1, 0), (2, 26, 42, 256, 256, 1, 1, 0), (3, 6, 10, 512, 128, 1, 1, 0)]
WS_ELIGIBILITY = [(2, 100, 168, 128, 512, 1, 1, 0), (1, 40, 50, 128, 512, 1, 1, 0), (2, 50, 84, 512, 256, 1, 1, 0), (2, 100, 168, 256, 256, 1, 1, 0),
                  (2, 50, 84, 1024, 256, 1, 1, 0), (2, 50, 84, 128, 384, 1, 1, 0), (2, 50, 84, 128, 512, 1, 1, 0)]
HALO64_SMALL = [(2, 25, 42, 64, 96, 3, 1, 1), (1, 19, 23, 128, 256, 3, 1, 1), (3, 9, 130, 64, 264, 3, 1, 1), (2, 13, 300, 192, 256, 3, 1, 1)]
HALO_KNOBS = [(4, 25, 42, 512, 512, 3, 1, 1), (2, 50, 84, 256, 256, 3, 1, 1), (1, 37, 41, 192, 256, 3, 1, 1), (2, 13, 21, 64, 512, 3, 1, 1)]
SPLITK = [(2048, 1, 1, 12544, 1024, 1, 1, 0), (1000, 1, 1, 12544, 1024, 1, 1, 0), (300, 1, 1, 4096, 256, 1, 1, 0), (130, 1, 1, 4096, 136, 1, 1, 0)]


def _uniq(seq):
    seen, out = set(), []
    for s in seq:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


SMALL_ALL = _uniq(SMALL + K64 + DIRECT_SMALL + WS_SMALL + HALO64_SMALL)
FORCE_SHAPES = _uniq(SMALL + K64[3:4] + WS_SMALL[:4])
FULL_TABLES = _uniq(FULL_FWD + DGRAD + DIRECT_FULL + WS_ELIGIBILITY + HALO_KNOBS + SPLITK)


def r50_fpn(N):
    """the R50-FPN layers (forward and data-gradient shapes) on the benchmark's padded 800 x 1344 input: stride-4 map 200 x 336"""
    out = []
    H, W = 200, 336
    cin = 64
    for stage, (mid, cout) in enumerate([(64, 256), (128, 512), (256, 1024), (512, 2048)]):
        s = 1 if stage == 0 else 2
        Ho, Wo = H // s, W // s
        out += [(N, H, W, cin, mid, 1, s, 0), (N, H, W, cin, cout, 1, s, 0),                     # first block: conv1 (stride in the 1x1), shortcut
                (N, Ho, Wo, mid, mid, 3, 1, 1), (N, Ho, Wo, mid, cout, 1, 1, 0),                 # conv2, conv3
                (N, Ho, Wo, cout, mid, 1, 1, 0),                                                  # conv1 of the later blocks = conv3's data gradient
                (N, Ho, Wo, mid, cin, 1, 1, 0), (N, Ho, Wo, cout, cin, 1, 1, 0),                 # data gradients of the strided conv1 / shortcut
                (N, Ho, Wo, cout, 256, 1, 1, 0), (N, Ho, Wo, 256, cout, 1, 1, 0),                # FPN lateral and its data gradient
                (N, Ho, Wo, 256, 256, 3, 1, 1), (N, Ho, Wo, 256, 16, 1, 1, 0), (N, Ho, Wo, 16, 256, 1, 1, 0)]      # FPN output / RPN conv, RPN heads
        H, W, cin = Ho, Wo, cout
    out += [(N, 13, 21, 256, 256, 3, 1, 1), (N, 13, 21, 256, 16, 1, 1, 0)]                        # p6
    R = 512 * N
    out += [(R, 1, 1, 12544, 1024, 1, 1, 0), (R, 1, 1, 1024, 12544, 1, 1, 0), (R, 1, 1, 1024, 1024, 1, 1, 0), (R, 1, 1, 1024, 48, 1, 1, 0),
            (R, 1, 1, 48, 1024, 1, 1, 0)]                                                         # box head FC1 / FC2 / predictors and data gradients
    return out


def token_linears():
    """ViT-B (768) and ConvNeXt-L (192 .. 1536) linears on the 800 x 1344 input"""
    out = []
    for N in (2, 4):
        M = N * 50 * 84
        out += [(M, 1, 1, 768, 2304, 1, 1, 0), (M, 1, 1, 768, 768, 1, 1, 0), (M, 1, 1, 768, 3072, 1, 1, 0), (M, 1, 1, 3072, 768, 1, 1, 0)]
        for lvl, c in enumerate((192, 384, 768, 1536)):
            out += [(N, 200 >> lvl, 336 >> lvl, c, 4 * c, 1, 1, 0), (N, 200 >> lvl, 336 >> lvl, 4 * c, c, 1, 1, 0)]
    return out


def detr_trunk():
    """fp32 Deformable-DETR: the R50 trunk at N = 2 and the input projections"""
    return [s for i, s in enumerate(r50_fpn(2)[:48]) if i % 12 < 7] + [(2, 100, 168, 512, 256, 1, 1, 0), (2, 50, 84, 1024, 256, 1, 1, 0), (2, 25, 42, 2048, 256, 1, 1, 0), (2, 25, 42, 2048, 256, 3, 2, 1)]


# ---------------------------------------------------------------------------------- problems
BF16_OPS = ["y", "y+relu", "y+scale+shift+relu", "y+scale+shift+relu+res1", "y+shift+res2", "y32", "y+res1+mask", "y+res1+mbits", "y+mbits", "y+scale+shift+relu+bout"]
F32_OPS = ["y", "y+scale+shift+relu", "y+scale+shift+relu+res1", "y+shift+res2", "y+mask"]


def out_hw(p):
    _, N, H, W, Cin, Cout, k, stride, pad = p[:9]
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def legal(p):
    """the argument rules of aldi_conv_igemm (fill_convdev, conv_splitk)"""
    dt, N, H, W, Cin, Cout, k, stride, pad, ops, ksplit, out_scale = p
    o = set(ops.split("+"))
    Ho, Wo = out_hw(p)
    bf = dt == "bf16"
    if (Cin % (8 if bf else 4)) if k == 1 else (Cin % (32 if bf else 16)):
        return False
    if Cout % 4 or Ho < 1 or Wo < 1:
        return False
    if "res2" in o and (Ho % 2 or Wo % 2):
        return False
    if ("mbits" in o or "bout" in o) and (not bf or Cout % 8 or out_scale != 1 or "res2" in o or "y" not in o or "y32" in o or ksplit > 1):
        return False
    if "mbits" in o and "mask" in o:
        return False
    esz = 2 if bf else 4
    if max(N * H * W * Cin, Cout * k * k * Cin, N * Ho * Wo * out_scale * out_scale * Cout) * esz >= 2 ** 31:
        return False
    if ksplit > 1 and (not bf or k != 1 or stride != 1 or pad or o & {"res1", "res2", "mask", "y32"} or out_scale > 1 or (k * k * Cin) % (64 * ksplit) or ksplit > 64):
        return False
    return True


def prob(dt, shape, ops, ksplit=0, out_scale=1):
    return [dt] + list(shape) + [ops, ksplit, out_scale]


PTR_FIELDS = ("x", "w", "y", "y_f32", "scale", "shift", "res", "mask", "ws", "mask_bits", "bits_out")


def conv_args(L, p, ptr):
    """aldi_conv_args of a problem; ptr: {field: address} (every PTR_FIELDS name) -- only the operands the problem names are set"""
    dt, N, H, W, Cin, Cout, k, stride, pad, ops, ksplit, out_scale = p
    o = set(ops.split("+"))
    Ho, Wo = out_hw(p)
    a = L.ConvArgs()
    a.x, a.w = ptr["x"], ptr["w"]
    a.y = ptr["y"] if "y" in o else None
    a.y_f32 = ptr["y_f32"] if "y32" in o else None
    a.scale = ptr["scale"] if "scale" in o else None
    a.shift = ptr["shift"] if "shift" in o else None
    a.res = ptr["res"] if o & {"res1", "res2"} else None
    a.mask = ptr["mask"] if "mask" in o else None
    a.mask_bits = ptr["mask_bits"] if "mbits" in o else None
    a.bits_out = ptr["bits_out"] if "bout" in o else None
    a.ws = ptr["ws"] if ksplit > 1 else None
    a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad, a.Ho, a.Wo = N, H, W, Cin, Cout, k, k, stride, pad, Ho, Wo
    a.relu = int("relu" in o)
    a.res_mode = 1 if "res1" in o else 2 if "res2" in o else 0
    a.out_scale = out_scale
    a.OH, a.OW = (Ho * out_scale, Wo * out_scale) if out_scale > 1 else (0, 0)
    a.dtype = L.BF16 if dt == "bf16" else L.F32
    a.ksplit = ksplit
    return a


def sizes(p):
    """bytes each buffer of a problem needs"""
    dt, N, H, W, Cin, Cout, k, stride, pad, ops, ksplit, out_scale = p
    Ho, Wo = out_hw(p)
    esz = 2 if dt == "bf16" else 4
    outs = N * Ho * Wo * out_scale * out_scale * Cout
    return {"x": N * H * W * Cin * esz, "w": Cout * k * k * Cin * esz, "y": outs * esz, "y_f32": outs * 4, "scale": Cout * 4, "shift": Cout * 4,
            "res": outs * esz, "mask": outs * esz, "ws": max(ksplit, 1) * N * Ho * Wo * Cout * 4 if ksplit > 1 else 0, "mask_bits": outs // 8 + 64,
            "bits_out": outs // 8 + 64}


# ---------------------------------------------------------------------------------- the sweep
def sweep():
    """-> [(case, knobs)]"""
    rows = []

    def single(p, knobs=None):
        if legal(p):
            rows.append((["s", p], dict(knobs or {})))

    def group(ps, knobs=None):
        if all(legal(p) for p in ps):
            rows.append((["g"] + ps, dict(knobs or {})))

    is3 = lambda s: s[5] == 3 and s[6] == 1 and s[7] == 1
    splitk_ok = lambda s: s[5] == 1 and s[6] == 1 and s[7] == 0 and s[3] % 256 == 0 and s[3] >= 2048 and s[0] * s[1] * s[2] * s[4] <= 1 << 23
    few = ("y+scale+shift+relu+res1", "y+res1+mbits")
    # defaults: the forward / direct tables with every operand set, the other tables with the operands their tests use, the rest with the step's two
    for s in FULL_TABLES:
        for ops in BF16_OPS if s in FULL_FWD + DIRECT_FULL else ("y", "y+relu", "y32", "y+scale+shift+relu"):
            single(prob("bf16", s, ops))
    for s in _uniq(SMALL_ALL + r50_fpn(4) + token_linears()):
        if s not in FULL_TABLES:
            for ops in few[:1] if s in SMALL_ALL else few:
                single(prob("bf16", s, ops))
    for s in _uniq(r50_fpn(2) + r50_fpn(6)):
        single(prob("bf16", s, "y+scale+shift+relu+res1"))
    for s in _uniq(FULL_TABLES + SMALL_ALL + r50_fpn(4)):
        if splitk_ok(s):
            for ops in ("y", "y+scale+shift+relu"):
                single(prob("bf16", s, ops, ksplit=4))
            for v in (0, 1, 3, 4) if s in FULL_TABLES + SMALL_ALL else ():
                single(prob("bf16", s, "y+scale+shift+relu", ksplit=4), {"igemm_splitk_tile": v})
    for s in _uniq(FULL_F32 + SMALL):
        for ops in F32_OPS:
            single(prob("f32", s, ops))
        single(prob("f32", s, "y+scale+shift+relu"), {"igemm_f32_tile64_max": 0})
        if is3(s):
            single(prob("f32", s, "y+scale+shift+relu"), {"igemm_halo_f32": 400})
    for s in detr_trunk():
        single(prob("f32", s, "y+scale+shift+relu+res1"))
    # scattered output (data gradient of a stride-2 1x1 conv)
    for (H, W, cg, cx) in ((100, 168, 512, 256), (100, 168, 128, 256), (50, 84, 1024, 512), (25, 42, 2048, 1024), (25, 42, 512, 1024)):
        for ops in ("y", "y+res1+mask"):
            single(prob("bf16", (4, H, W, cg, cx, 1, 1, 0), ops, out_scale=2))
        single(prob("f32", (2, H, W, cg, cx, 1, 1, 0), "y+res1", out_scale=2))
    # igemm_force: every arm on the small shapes
    for f in range(1, 18):
        for s in FORCE_SHAPES:
            single(prob("bf16", s, "y+scale+shift+relu"), {"igemm_force": f})
            if s in (SMALL[0], SMALL[3]):
                for ops in ("y+scale+shift+relu+res1", "y+mbits"):
                    single(prob("bf16", s, ops), {"igemm_force": f})
            if s in SMALL[:5] and f <= 5:
                single(prob("f32", s, "y+scale+shift+relu"), {"igemm_force": f})
                if f in (1, 2, 4) and is3(s):
                    single(prob("f32", s, "y"), {"igemm_force": f, "igemm_halo_f32": 1})        # the fp32 halo tiles: two knobs
        single(prob("bf16", SPLITK[3], "y+scale+shift+relu", ksplit=4), {"igemm_force": f})
    # each non-default arm, one at a time
    k3 = [("igemm_halo", 0), ("igemm_bigtile", 1), ("igemm_bigtile", 10), ("igemm_bigtile", 65), ("igemm_halo64_mid", 200), ("igemm_halo64_mid", 256),
          ("igemm_halo96", 1), ("igemm_halo_small", 320), ("igemm_halo_ilv", 0)]
    k1 = [("igemm_tile", 7), ("igemm_tile", 9), ("igemm_ws", 0), ("igemm_lean", 0)]
    for s in FULL_TABLES:
        for name, v in (k3 if is3(s) else k1 if s[5] == 1 and s in FULL_FWD + DIRECT_FULL else []):
            single(prob("bf16", s, "y+relu" if is3(s) else "y+scale+shift+relu"), {name: v})
        for ops in ("y+scale+shift+relu+res1", "y+res1+mbits") if s in FULL_FWD + DIRECT_FULL else ():
            single(prob("bf16", s, ops), {"igemm_direct": 0})
    for s in WS_ELIGIBILITY:
        for ops in ("y", "y+res2", "y+scale+shift+relu"):
            single(prob("bf16", s, ops), {"igemm_ws_min": 4096})
    # threshold knobs: one value on either side of the shape's own count
    for s, name, count in (((4, 100, 168, 256, 256, 3, 1, 1), "igemm_bigtile_min", 1050),            # 525 x 2 tiles of 128 x 128
                           ((1, 120, 140, 3072, 768, 1, 1, 0), "igemm_lintile_min", 792),             # 132 x 6
                           ((1, 120, 140, 3072, 768, 1, 1, 0), "igemm_bigtile_k", 3072),
                           ((4, 50, 84, 1024, 256, 1, 1, 0), "igemm_k64_min", 1024),
                           ((4, 25, 42, 512, 2048, 1, 1, 0), "igemm_narrow_k", 512),              # 33 x 16 tiles, below igemm_ws_min: the narrow-K rule decides
                           ((4, 100, 168, 128, 512, 1, 1, 0), "igemm_ws_min", 67200)):
        for v in (count, count + 1, count - 1):
            single(prob("bf16", s, "y+scale+shift+relu"), {name: v})
    for v in (263, 264, 265):
        single(prob("f32", (2, 100, 168, 128, 128, 3, 1, 1), "y"), {"igemm_f32_tile64_max": v})      # 263 x 1 tiles
    for v in (525, 526, 527):
        single(prob("f32", (2, 100, 168, 128, 128, 3, 1, 1), "y"), {"igemm_halo_f32": v})            # 263 x 2 half-width tiles
    # groups
    pyr5 = [(2, 200, 336), (2, 100, 168), (2, 50, 84), (2, 25, 42), (2, 13, 21)]
    pyr9 = [(4, 100, 168), (4, 50, 84), (4, 25, 42), (4, 13, 21), (2, 100, 168), (2, 50, 84), (2, 25, 42), (2, 13, 21), (1, 7, 11)]
    for kn in ({}, {"igemm_group": 0}, {"igemm_bigtile": 4}, {"igemm_direct": 0}, {"igemm_halo_ilv": 0}, {"igemm_force": 11}):
        for k, pad in ((3, 1), (1, 0)):
            for ops in ("y+shift+relu", "y32"):
                group([prob("bf16", (N, H, W, 256, 256, k, 1, pad), ops) for (N, H, W) in pyr5], kn)
            group([prob("bf16", (N, H, W, 256, 256, k, 1, pad), "y+shift+relu") for (N, H, W) in pyr9], kn)
            group([prob("bf16", (N, H, W, 256, 256, k, 1, pad), "y+shift+relu" if i else "y+shift+relu+bout") for i, (N, H, W) in enumerate(pyr5)], kn)
            group([prob("f32", (N, H, W, 256, 256, k, 1, pad), "y+shift+relu") for (N, H, W) in pyr5[1:]], kn)
        for geo in ((50, 84, 256, 256, 3, 1, 1), (200, 336, 256, 256, 3, 1, 1), (100, 168, 256, 256, 3, 1, 1), (50, 84, 1024, 256, 1, 1, 0), (25, 42, 1024, 2048, 1, 2, 0),
                    (13, 21, 256, 16, 1, 1, 0), (100, 168, 128, 512, 1, 1, 0)):
            group([prob("bf16", (N,) + geo, "y+scale+shift+relu+res1") for N in (4, 2)], kn)         # student + teacher
        group([prob("bf16", (N, 19, 23, 64, 96, 3, 1, 1), "y+scale+shift+relu+res1") for N in (3, 1, 2)], kn)
        group([prob("bf16", SMALL[0], "y"), prob("bf16", SMALL[3], "y")], kn)                        # different layers: single launches
        group([prob("bf16", SMALL[0], "y")], kn)                                                     # n = 1
    group([prob("bf16", (N, H, W, 256, 256, 3, 1, 1), "y+shift+relu") for (N, H, W) in pyr9 + pyr9[:4]])      # more than 12 problems
    seen, out = set(), []
    for case, knobs in rows:
        key = json.dumps([case, knobs], sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append((case, knobs))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--time-limit", type=float, default=600.0, help="seconds; past it the run stops with exit code 3")
    ap.add_argument("--count", action="store_true", help="print the number of rows of the sweep and exit (no GPU)")
    a = ap.parse_args()
    rows = sweep()
    if a.count:
        print(len(rows))
        return 0
    import torch
    from aldi_amd import _lib as L
    need = {f: 0 for f in PTR_FIELDS}
    for case, _ in rows:
        for p in case[1:]:
            for f, b in sizes(p).items():
                need[f] = max(need[f], b)
    bufs = {f: torch.zeros(max(b, 64), dtype=torch.uint8, device="cuda") for f, b in need.items()}
    ptr = {f: t.data_ptr() for f, t in bufs.items()}
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.time()
    table = []
    for case, knobs in rows:
        if time.time() - t0 > a.time_limit:
            print("time limit after %d of %d rows" % (len(table), len(rows)), file=sys.stderr)
            return 3
        L.lib.aldi_reset_tuning()
        for k, v in knobs.items():
            if L.lib.aldi_set_tuning(k.encode(), int(v)):
                print("unknown knob", k, file=sys.stderr)
                return 2
        if case[0] == "s":
            arg = conv_args(L, case[1], ptr)
            rc = L.lib.aldi_conv_igemm(C.byref(arg), stream)
        else:
            arr = (L.ConvArgs * (len(case) - 1))(*[conv_args(L, p, ptr) for p in case[1:]])
            rc = L.lib.aldi_conv_igemm_group(arr, len(case) - 1, stream)
        if rc:
            print("status %d (%s) at %s %s" % (rc, L.lib.aldi_last_error().decode(), case, knobs), file=sys.stderr)
            return 1
        name = L.lib.aldi_last_dispatch().decode()
        torch.cuda.synchronize()            # a fault surfaces here, at the row that caused it: nothing more is launched
        table.append([case, knobs, name])
    L.lib.aldi_reset_tuning()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in table) + "\n]\n")
    print("%d rows, %d distinct kernels, %.1f s" % (len(table), len({r[2] for r in table}), time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Operands and plain fp64 references for the kernel-level tests of the token kernels of the ViTDet and ConvNeXt detectors
(csrc/vit.hip, csrc/convnext.hip): LayerNorm forward / backward, GELU, the row gather-add, patch extraction, the two resamplers, add_pos /
sum_batch, the 2 x 2 max pool, AdamW, the depthwise 7 x 7 convolution with both gradients and the layer-scale add.

Two kinds of check, as in detr_kernel_refs.py and roialign_exact.py:

  exact          lattice operands (small integers, powers of two, quarters) on which every product and every sum is exact in fp32 in any order,
                 with or without a fused multiply-add: the kernel is held to torch.equal with the explicit fp64 reference rounded ONCE to the output
                 dtype (the one bf16 rounding is round-to-nearest-even of an exactly representable fp32 value).  The `check_*` functions assert on
                 the reference side that the construction really is exact: per output element sum |terms| < 2^24 x the terms' granularity.
  fp64-matched   the truth is the reference in fp64 on the kernel's own operands (already rounded to bf16 / fp32, hyper-parameters already rounded to
                 fp32), the yardstick is the same function in fp32 on the CPU, and a kernel may be FACTOR times as far from the truth as the yardstick
                 plus four ulps of the largest entry (`tolerance`); a bf16 output may add half a bf16 ulp of each reference element.

The host-side launch arithmetic the tests aim at (rows per block, chunks, rows left for the tail loops) is restated in the `*_plan` functions, so that
the CPU tests can assert that the chosen shapes and knobs reach the paths they are meant to reach.

Nothing here touches the library under test.  Shared by test_token_kernels_cpu.py and test_token_kernels_gpu.py."""
import functools
import math

import torch

FACTOR = 8.0


# ------------------------------------------------------------------------------------------------ the rules
def tolerance(ref32, ref64, factor=FACTOR):
    """a kernel may be `factor` times as far from the fp64 truth as the same function in fp32 on the CPU, plus four ulps of the largest entry"""
    return factor * (ref32.double() - ref64).abs().max().item() + 4 * 2.0 ** -24 * ref64.abs().max().item()


def both(fn, *operands, **kw):
    """-> (fn in fp32, fn in fp64) on the same operands; tensors of other dtypes and non-tensors pass through"""
    def cast(dt):
        return [o.to(dt) if torch.is_tensor(o) and o.is_floating_point() else o for o in operands]
    return fn(*cast(torch.float32), **kw), fn(*cast(torch.float64), **kw)


def bf16_half_ulp(ref):
    """half a bf16 ulp of each reference value (8 significant bits: ulp = 2^(e - 7) for 2^e <= |v| < 2^(e + 1))"""
    e = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126)))
    return 2.0 ** (e - 8)


def round_to(ref64, dtype):
    """the fp64 reference rounded once to the output dtype (the value has to be an fp32 number for the bf16 rounding to be a single one)"""
    r32 = ref64.float()
    assert torch.equal(r32.double(), ref64), "the reference is not representable in fp32"
    return r32.to(dtype)


def on_lattice(t, unit):
    """every entry of t is a multiple of `unit`"""
    return bool(torch.equal(t.double() / unit, (t.double() / unit).round()))


def budget(abs_sum, granularity):
    """share of the exactness budget in use: an fp32 sum of multiples of `granularity` is exact in any order while sum |terms| < 2^24 granularity"""
    return float(abs_sum.max().item()) / (2.0 ** 24 * granularity)


def f32(v):
    """a Python number rounded to fp32 (what a kernel receives for a float argument)"""
    return float(torch.tensor(v, dtype=torch.float32))


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def choice(g, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def partition_map(N, gh, gw, ws):
    """window-order row map (detectron2 window_partition): output row -> source token or -1 (padding)"""
    ph, pw = (ws - gh % ws) % ws, (ws - gw % ws) % ws
    Hp, Wp = gh + ph, gw + pw
    idx = torch.full((N, Hp, Wp), -1, dtype=torch.int32)
    idx[:, :gh, :gw] = torch.arange(N * gh * gw, dtype=torch.int32).view(N, gh, gw)
    return idx.view(N, Hp // ws, ws, Wp // ws, ws).permute(0, 1, 3, 2, 4).reshape(-1).contiguous()


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_C_BF16_WIDE = (8, 64, 512, 520, 1024, 1032, 2048)     # the 8-wide forms: 512 / 1024 / 2048 end the 1- / 2- / 4-chunk form, 520 / 1032 leave one live lane in the last chunk
LN_C_BF16_NARROW = (4, 100, 1028)                        # rows that are not whole 16-B vectors: the 4-wide form
LN_C_F32 = (4, 100, 1024, 1028, 2048)
LN_ROWS = (1, 3, 333, 1025)
LN_EPS = 1e-6
LN_MAP = (2, 5, 6, 4)                                    # N, gh, gw, window: 60 tokens in 2 x 2 x 2 windows of 16 rows, 68 of the 128 rows are padding


def is_pow2(n):
    return n >= 1 and n & (n - 1) == 0


def ln_bwd_plan(rows, target_blocks):
    """(rows per block, blocks, rows of the last block) of aldi_layernorm_backward for the knob ln_bwd_blocks(_narrow) = target_blocks"""
    rpb = max(32, -(-rows // target_blocks))
    blocks = -(-rows // rpb)
    return rpb, blocks, rows - (blocks - 1) * rpb


def ln_bwd_operands(rows, C, seed, use_map=False):
    """integer mean, rstd in {1, 2}, integer x with |x - mean| <= 4, g in {-1, 0, 1}, gamma in {0.5, 1, 2}, integer res with |res| <= 4, mask in
    {0, 1}: everything bf16-representable.  use_map: `rows` is ignored, the rows are those of the window partition LN_MAP; g, mask, mean, rstd
    are indexed by the output (window) row, x, res and dx by the source token; the padding rows carry g = 1 and NaN statistics."""
    g_ = torch.Generator().manual_seed(seed)
    if use_map:
        row_map = partition_map(*LN_MAP)
        n_src, rows = LN_MAP[0] * LN_MAP[1] * LN_MAP[2], row_map.numel()
    else:
        row_map, n_src = None, rows
    mean_src = ints(g_, (n_src,), -8, 8)
    rstd_src = choice(g_, (n_src,), (1.0, 2.0))
    x = mean_src[:, None] + ints(g_, (n_src, C), -4, 4)
    res = ints(g_, (n_src, C), -4, 4)
    g = ints(g_, (rows, C), -1, 1)
    mask = ints(g_, (rows, C), 0, 1)
    gamma = choice(g_, (C,), (0.5, 1.0, 2.0))
    if use_map:
        valid = row_map >= 0
        mean, rstd = torch.full((rows,), float("nan")), torch.full((rows,), float("nan"))
        mean[valid], rstd[valid] = mean_src[row_map[valid].long()], rstd_src[row_map[valid].long()]
        g[~valid] = 1.0
        mask[~valid] = 1.0
    else:
        mean, rstd = mean_src, rstd_src
    return dict(g=g, x=x, gamma=gamma, mean=mean, rstd=rstd, res=res, mask=mask, row_map=row_map)


def ln_bwd_ref(g, x, gamma, mean, rstd, res=None, mask=None, row_map=None, absolute=False):
    """dx[src] = rstd * (g gamma - mean_c(g gamma) - xhat mean_c(g gamma xhat)) (+ res[src]), dgamma = sum_r g xhat, dbeta = sum_r g, with
    g -> g * (mask > 0) first and the rows with row_map < 0 left out; in the operands' dtype.
    absolute: every magnitude and every difference replaced by a sum -> (the widest intermediate of dx before the factor rstd, sum |g xhat|, sum |g|)"""
    C = x.shape[1]
    src = torch.arange(g.shape[0]) if row_map is None else row_map.long()
    valid = src >= 0
    gv = g if mask is None else torch.where(mask > 0, g, torch.zeros_like(g))
    gv, mu, rs = gv[valid], mean[valid][:, None], rstd[valid][:, None]
    xh = (x[src[valid]] - mu) * rs
    if absolute:
        gv, xh, gamma = gv.abs(), xh.abs(), gamma.abs()
    gg = gv * gamma
    s1, s2 = gg.sum(1, keepdim=True) / C, (gg * xh).sum(1, keepdim=True) / C
    if absolute:
        return gg + s1 + xh * s2, (gv * xh).sum(0), gv.sum(0), gg.sum(1), (gg * xh).sum(1)
    d = rs * (gg - s1 - xh * s2)
    dx = torch.zeros_like(x)
    dx[src[valid]] = d
    if res is not None:
        dx = dx + res
    return dict(dx=dx, dgamma=(gv * xh).sum(0), dbeta=gv.sum(0))


def check_ln_bwd(ops, res=True, mask=True):
    """the preconditions of the exact LayerNorm-backward tests -> the bits the widest intermediate needs (dx is exact for a power-of-two C only).
    Terms: g xhat and g are integers (dgamma, dbeta); g gamma and g gamma xhat are multiples of 1/2 (the two wave sums); after the division by a
    power-of-two C the three terms of dx are multiples of 1 / (2 C)."""
    C = ops["x"].shape[1]
    valid = torch.ones(ops["g"].shape[0], dtype=torch.bool) if ops["row_map"] is None else ops["row_map"] >= 0
    for k, unit in (("g", 1), ("x", 1), ("res", 1), ("mask", 1), ("gamma", 0.5)):
        assert on_lattice(ops[k], unit), k
        assert torch.equal(ops[k], ops[k].bfloat16().float()), k
    assert on_lattice(ops["mean"][valid], 1) and set(ops["rstd"][valid].tolist()) <= {1.0, 2.0}
    assert set(ops["gamma"].tolist()) <= {0.5, 1.0, 2.0} and ops["g"].abs().max() <= 1 and ops["res"].abs().max() <= 4
    src = torch.arange(ops["g"].shape[0]) if ops["row_map"] is None else ops["row_map"].long()
    assert ((ops["x"][src[valid]] - ops["mean"][valid][:, None]).abs() <= 4).all()
    d = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in ops.items()}
    wide, a_dg, a_db, a_s1, a_s2 = ln_bwd_ref(d["g"], d["x"], d["gamma"], d["mean"], d["rstd"], None, d["mask"] if mask else None, d["row_map"], absolute=True)
    use = max(budget(a_dg, 1.0), budget(a_db, 1.0), budget(a_s1, 0.5), budget(a_s2, 0.5))
    if is_pow2(C):
        use = max(use, budget(wide, 0.5 / C))
    assert use < 1.0, use
    return 24 + math.log2(use)


@functools.lru_cache(maxsize=None)
def ln_bwd_case(rows, C, res, mask, use_map=False):
    """operands, fp64 reference and the same reference in fp32 (the yardstick of dx where C is no power of two); computed once, never modified"""
    ops = ln_bwd_operands(rows, C, 1000 * C + rows + 7 * use_map, use_map)
    bits = check_ln_bwd(ops, res, mask)
    r32, r64 = both(ln_bwd_ref, ops["g"], ops["x"], ops["gamma"], ops["mean"], ops["rstd"], ops["res"] if res else None, ops["mask"] if mask else None, ops["row_map"])
    return ops, r64, r32, bits


LN_FWD_KINDS = ("randn", "randn+30", "1e-3*randn+100", "outlier")


def ln_fwd_operands(C, seed, dtype, rows_per_kind=5):
    """rows of randn, randn + 30, 1e-3 randn + 100 and randn with a single 1e4 outlier, rounded to the kernel's dtype -> x, gamma, beta (fp32 values)"""
    g_ = torch.Generator().manual_seed(seed)
    n = rows_per_kind
    x = torch.randn(4 * n, C, generator=g_)
    x[n:2 * n] += 30
    x[2 * n:3 * n] = 1e-3 * x[2 * n:3 * n] + 100
    x[3 * n:] = torch.where(torch.arange(C)[None, :] == (torch.arange(n) * 7 % C)[:, None], torch.full((n, C), 1e4), torch.randn(n, C, generator=g_))
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g_), torch.randn(C, generator=g_)
    return x.to(dtype).float(), gamma, beta


def ln_fwd_ref(x, gamma, beta, eps=LN_EPS, row_map=None, relu=False):
    """two-pass LayerNorm over the last axis -> y, mean, rstd; row_map: output row r normalises source row row_map[r], -1 gives a zero row with
    mean = rstd = 0; relu: y clamped at 0.  eps is the fp32 number the kernel receives."""
    eps = f32(eps)
    if row_map is not None:
        valid = row_map >= 0
        x = x[row_map.clamp(min=0).long()]
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1 / torch.sqrt((xc * xc).mean(1, keepdim=True) + eps)
    y = xc * rstd * gamma + beta
    if relu:
        y = y.clamp_min(0)
    mean, rstd = mean[:, 0], rstd[:, 0]
    if row_map is not None:
        y, mean, rstd = y * valid[:, None], mean * valid, rstd * valid
    return dict(y=y, mean=mean, rstd=rstd)


# ------------------------------------------------------------------------------------------------ GELU
GELU_SPECIAL = (20.0, 100.0, 1e4)
GELU_FAR = 9000.0                                         # 1e4 is 9984 in bf16: from here on the output is exactly x or a zero
GELU_AS_BOUND = 1.5e-7                                    # Abramowitz-Stegun 7.1.26: |error| of erf


def bf16_values(limit=10.0):
    """every finite bf16 value of magnitude <= limit, both zeros and the subnormals included, as fp32"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16).float()
    return v[torch.isfinite(v) & (v.abs() <= limit)]


def gelu_inputs(extra_grid=0):
    """all bf16 values in [-10, 10], +-20, +-100, +-1e4 (rounded to bf16) and the largest finite bf16 of either sign (+ an fp32 grid of
    `extra_grid` points over [-10, 10]) -> x (fp32, a multiple of 8 long: padded with 0.5) and an upstream gradient g (bf16 values, none zero)"""
    big = torch.tensor(GELU_SPECIAL + (torch.finfo(torch.bfloat16).max,)).bfloat16().float()
    parts = [bf16_values(), big, -big]
    if extra_grid:
        parts.append(torch.linspace(-10, 10, extra_grid))
    x = torch.cat(parts)
    x = torch.cat([x, torch.full(((-x.numel()) % 8,), 0.5)])
    g_ = torch.Generator().manual_seed(5)
    g = (torch.randn(x.numel(), generator=g_) + torch.tensor(3.0)).bfloat16().float()
    g = torch.where(g == 0, torch.ones_like(g), g) * torch.where(torch.arange(x.numel()) % 2 == 0, 1.0, -1.0)
    return x, g


def gelu_ref(x, g=None):
    """x Phi(x) (g None) or g (Phi(x) + x phi(x)), Phi through erfc: no cancellation in the negative tail"""
    cdf = 0.5 * torch.erfc(-x * math.sqrt(0.5))
    if g is None:
        return x * cdf
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return g * (cdf + x * pdf)


def gelu_torch(x, g=None):
    """F.gelu and its autograd in x's dtype"""
    if g is None:
        return torch.nn.functional.gelu(x)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xr).backward(g)
    return xr.grad


def gelu_bands(x):
    """a band number per element: the sign of x and the binade of |x| (everything up to 1/4 in one band, 2^-2 < |x| <= 2^-1, ..., 64 < |x| <= 128);
    0 for |x| >= GELU_FAR, where the output is held to exact equality instead"""
    k = torch.ceil(torch.log2(x.abs().double().clamp(min=2.0 ** -2))).clamp(max=7).long() + 3          # 1 .. 10
    band = torch.where(x < 0, -k, k)
    return torch.where(x.abs() >= GELU_FAR, torch.zeros_like(band), band)


def gelu_allowed(x, g, lowp):
    """per element: 1.5e-7 max(1, |x|) (|g|) + `tolerance` of the fp32 F.gelu yardstick (+ half a bf16 ulp of the truth); the yardstick's
    tolerance is taken per band of x (sign and binade), so that its largest error and the four ulps of the largest entry are those of the
    element's own neighbourhood and not of the whole tensor, whose maximum is seven orders above the tail.
    -> truth, allowed, the mask of the banded elements (|x| < GELU_FAR)"""
    x64 = x.double()
    g64 = None if g is None else g.double()
    truth = gelu_ref(x64, g64)
    y32 = gelu_torch(x.float(), None if g is None else g.float())
    allowed = GELU_AS_BOUND * x64.abs().clamp(min=1) * (1 if g is None else g64.abs())
    band = gelu_bands(x)
    for b in band.unique().tolist():
        if b != 0:
            m = band == b
            allowed[m] += tolerance(y32[m], truth[m])
    banded = band != 0
    if lowp:
        allowed = allowed + bf16_half_ulp(truth)
    return truth, allowed, banded


# ------------------------------------------------------------------------------------------------ the small kernels
def rows_add_ref(a, b, row_map=None, scale=None, rows_per_sample=1, rows=None):
    """out[r] = (a ? a[r] : 0) + s(r) (idx >= 0 ? b[idx] : 0), idx = row_map ? row_map[r] : r, s(r) = scale ? scale[r // rows_per_sample] : 1"""
    rows = rows if rows is not None else (row_map.numel() if row_map is not None else b.shape[0])
    idx = torch.arange(rows) if row_map is None else row_map.long()
    bv = b[idx.clamp(min=0)] * (idx >= 0)[:, None]
    if scale is not None:
        bv = bv * scale[torch.arange(rows) // rows_per_sample][:, None]
    return bv if a is None else a + bv


PIXEL_MEAN, PIXEL_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def patchify_operands(P, seed):
    """three images of 50 x 70, 64 x 96 and 61 x 93 pixels in a 64 x 96 staging buffer whose bytes outside each image are 255"""
    g_ = torch.Generator().manual_seed(seed)
    hw = torch.tensor([[50, 70], [64, 96], [61, 93]], dtype=torch.int32)
    img = torch.randint(0, 256, (3, 3, 64, 96), generator=g_, dtype=torch.uint8)
    for n, (h, w) in enumerate(hw.tolist()):
        img[n, :, h:, :] = 255
        img[n, :, :, w:] = 255
    return img, hw


def patchify_ref(img, hw, P, mean=PIXEL_MEAN, std=PIXEL_STD, dtype=torch.float32):
    """((float) u8 - mean) * (1.f / std) inside image n, 0 outside, as rows [N gh gw][3 P P] in (c, py, px) order; in fp32 (dtype float32: the
    kernel's own expression, bit for bit) or in fp64 on the fp32 mean and fp32 1 / std"""
    N, _, Hs, Ws = img.shape
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    inv = (torch.ones(3, dtype=torch.float32) / torch.tensor(std, dtype=torch.float32)).view(1, 3, 1, 1)
    xn = (img.to(dtype) - m.to(dtype)) * inv.to(dtype)
    ys, xs = torch.arange(Hs).view(1, 1, Hs, 1), torch.arange(Ws).view(1, 1, 1, Ws)
    inside = (ys < hw[:, 0].view(N, 1, 1, 1)) & (xs < hw[:, 1].view(N, 1, 1, 1))
    xn = torch.where(inside, xn, torch.zeros_like(xn))
    gh, gw = Hs // P, Ws // P
    return xn.view(N, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, 3 * P * P)


# (L0, L1): identity, a one-entry and a two-entry table, one output, x2 up, 3:1 down, the model's own ratios
LINEAR_CASES = ((27, 27), (1, 1), (1, 5), (2, 7), (5, 1), (7, 14), (27, 9), (127, 99), (5, 11))
# (S0h, S0w, gh, gw): identity (square and not), a one-pixel and a two-pixel source, one output, x2 up, 3:1 down, non-square sources
BICUBIC_CASES = ((4, 4, 4, 4), (3, 5, 3, 5), (1, 1, 3, 4), (2, 2, 5, 5), (3, 5, 1, 1), (3, 5, 6, 10), (9, 6, 3, 2), (5, 2, 7, 3), (3, 5, 8, 7), (14, 14, 9, 13))


def source_coord(n_in, n_out, coord=torch.float32):
    """(i + 0.5) * (n_in / n_out) - 0.5 for every output index, evaluated in `coord` (fp32: the kernel's own coordinate)"""
    scale = torch.tensor(float(n_in), dtype=coord) / torch.tensor(float(n_out), dtype=coord)
    return (torch.arange(n_out, dtype=coord) + 0.5) * scale - 0.5


def linear_weights(L0, L1, dtype=torch.float64, coord=torch.float32):
    """the tap-weight matrix [L1][L0] of F.interpolate(mode="linear", align_corners=False): weights in `dtype` from the `coord` coordinate"""
    src = source_coord(L0, L1, coord).clamp(min=0)
    i0 = src.long()
    i1 = i0 + (i0 < L0 - 1).long()
    lam = (src - i0.to(coord)).to(dtype)
    W = torch.zeros(L1, L0, dtype=dtype)
    W.index_put_((torch.arange(L1), i0), 1 - lam, accumulate=True)
    W.index_put_((torch.arange(L1), i1), lam, accumulate=True)
    return W


def cubic_weights(n_in, n_out, dtype=torch.float64, coord=torch.float32):
    """the tap-weight matrix [n_out][n_in] of one axis of F.interpolate(mode="bicubic", align_corners=False): A = -0.75, border indices clamped"""
    A = -0.75
    s = source_coord(n_in, n_out, coord)
    f = torch.floor(s)
    t = (s - f).to(dtype)
    x0, x1, x2, x3 = t + 1, t, 1 - t, 2 - t
    w = [((A * x0 - 5 * A) * x0 + 8 * A) * x0 - 4 * A, ((A + 2) * x1 - (A + 3)) * x1 * x1 + 1,
         ((A + 2) * x2 - (A + 3)) * x2 * x2 + 1, ((A * x3 - 5 * A) * x3 + 8 * A) * x3 - 4 * A]
    W = torch.zeros(n_out, n_in, dtype=dtype)
    for k in range(4):
        W.index_put_((torch.arange(n_out), (f.long() - 1 + k).clamp(0, n_in - 1)), w[k], accumulate=True)
    return W


def linear_ref(t, L1, backward_into=None):
    """forward: W t [L1][C]; backward (t = the gradient [L1][C], backward_into = L0): W^T t; in t's dtype"""
    if backward_into is None:
        return linear_weights(t.shape[0], L1, t.dtype) @ t
    return linear_weights(backward_into, L1, t.dtype).t() @ t


def bicubic_ref(t, gh, gw, backward_into=None):
    """forward: t [S0h][S0w][C] -> [gh][gw][C]; backward (t = the gradient [gh][gw][C], backward_into = (S0h, S0w)): the transpose"""
    if backward_into is None:
        Wy, Wx = cubic_weights(t.shape[0], gh, t.dtype), cubic_weights(t.shape[1], gw, t.dtype)
        return torch.einsum("ya,xb,abc->yxc", Wy, Wx, t)
    Wy, Wx = cubic_weights(backward_into[0], gh, t.dtype), cubic_weights(backward_into[1], gw, t.dtype)
    return torch.einsum("ya,xb,yxc->abc", Wy, Wx, t)


MAXPOOL_C = 8


def maxpool_operands():
    """x (1, 2, 2 W, C) NHWC whose 2 x 2 windows enumerate: the 15 tie patterns (the maximum 1 on a non-empty subset of the taps, the rest 0,
    and the same with the rest -1 / -2 in the other channels), +0.0 against -0.0 in all 16 arrangements, -inf everywhere, and a NaN in each of the
    four taps (over finite values and over +inf) -> x, the upstream gradient g (never zero)"""
    wins = []
    for s in range(1, 16):
        wins.append([1.0 if s >> t & 1 else 0.0 for t in range(4)])
    for s in range(16):
        wins.append([0.0 if s >> t & 1 else -0.0 for t in range(4)])
    wins.append([float("-inf")] * 4)
    for t in range(4):
        for rest in (2.0, float("inf")):
            w = [rest, 1.0, 3.0, rest]
            w[t] = float("nan")
            wins.append(w)
    w = torch.tensor(wins)                                            # (n, 4)
    n = w.shape[0]
    x = torch.empty(1, 2, 2 * n, MAXPOOL_C)
    for c in range(MAXPOOL_C):
        wc = w.clone()
        if c % 4 == 1:                                                # the losers lower and distinct: the tie is among the winners only
            lose = (w == 0) & (torch.arange(n)[:, None] < 15)
            wc = torch.where(lose, -1.0 - torch.arange(4.0)[None, :], w)
        elif c % 4 == 2:                                              # the window mirrored: taps 3, 2, 1, 0
            wc = w.flip(1)
        elif c % 4 == 3:                                              # rows swapped: taps 2, 3, 0, 1
            wc = w[:, [2, 3, 0, 1]]
        x[0, :, :, c] = wc.view(n, 2, 2).permute(1, 0, 2).reshape(2, 2 * n)
    g_ = torch.Generator().manual_seed(9)
    g = ints(g_, (1, 1, n, MAXPOOL_C), 1, 4) * choice(g_, (1, 1, n, MAXPOOL_C), (-1.0, 1.0))
    return x, g


def maxpool_ref(x):
    """NHWC 2 x 2 / 2 max pool, written out: the first maximum in row-major window order wins, a NaN beats everything before it
    -> values (N, H/2, W/2, C), tap (uint8: 2 dy + dx)"""
    N, H, W, C = x.shape
    taps = [x[:, dy::2, dx::2, :] for dy in (0, 1) for dx in (0, 1)]
    best, tap = taps[0].clone(), torch.zeros(taps[0].shape, dtype=torch.uint8)
    for t in range(1, 4):
        take = (taps[t] > best) | torch.isnan(taps[t])
        best = torch.where(take, taps[t], best)
        tap = torch.where(take, torch.full_like(tap, t), tap)
    return best, tap


def maxpool_torch(x):
    """F.max_pool2d(return_indices=True) on the same map -> values NHWC, tap (uint8) from the flat input index"""
    N, H, W, C = x.shape
    y, idx = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 2, 2, return_indices=True)
    iy, ix = idx // W, idx % W
    ho, wo = torch.arange(H // 2).view(1, 1, -1, 1), torch.arange(W // 2).view(1, 1, 1, -1)
    tap = (iy - 2 * ho) * 2 + (ix - 2 * wo)
    assert ((tap >= 0) & (tap < 4)).all()
    return y.permute(0, 2, 3, 1).contiguous(), tap.permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def maxpool_bwd_ref(g, tap, H, W):
    """dx (N, H, W, C): g at the recorded tap, 0 elsewhere"""
    N, Ho, Wo, C = g.shape
    dx = torch.zeros(N, H, W, C, dtype=g.dtype)
    for t in range(4):
        dx[:, t >> 1::2, t & 1::2, :] = torch.where(tap == t, g, torch.zeros_like(g))
    return dx


def same_bits(a, b):
    """equal values with equal signs of zero; NaN matches NaN"""
    a, b = a.float(), b.float()
    return bool((torch.isnan(a) == torch.isnan(b)).all() and torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0)) and torch.equal(torch.signbit(a) | torch.isnan(a), torch.signbit(b) | torch.isnan(b)))


ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.1)
ADAMW_STEPS = (1, 2, 3, 1000, 100000)


def adamw_hyper(grad_scale=1.0):
    """the hyper-parameters as the fp32 numbers the kernel receives"""
    h = {k: f32(v) for k, v in ADAMW_HYPER.items()}
    h["grad_scale"] = f32(grad_scale)
    return h


def adamw_operands(n, seed, late):
    """p, g, m, v (fp32); late: m and v as they are after many steps, otherwise zero; the first element (and every 97th) has g = 0 and v = 0"""
    g_ = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    m = 0.1 * torch.randn(n, generator=g_) if late else torch.zeros(n)
    v = 0.01 * torch.rand(n, generator=g_) if late else torch.zeros(n)
    g[::97], v[::97], m[::97] = 0.0, 0.0, 0.0
    return p, g, m, v


def adamw_ref(p, g, m, v, step, lr, beta1, beta2, eps, wd, grad_scale=1.0):
    """one step of torch.optim.AdamW (decoupled decay, bias-corrected) on g * grad_scale, in p's dtype -> p, m, v"""
    g = g * grad_scale
    p = p * (1 - lr * wd)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return dict(p=p - (lr / bc1) * (m / denom), m=m, v=v)


# ------------------------------------------------------------------------------------------------ depthwise 7 x 7
DW_SHAPES = ((1, 1, 1), (2, 1, 9), (2, 3, 5), (1, 7, 7), (2, 8, 13), (2, 5, 12), (2, 13, 17))       # (N, H, W)
DW_CHANNELS = (8, 24, 200, 264)


def dw_groups(C):
    """(channel groups of 8, groups per block CG, blocks along the channels) of aldi_dwconv7_wgrad / aldi_scale_add_backward"""
    c8 = C // 8
    CG = 32 if c8 >= 32 else 16 if c8 >= 16 else 8 if c8 >= 8 else 4 if c8 >= 4 else 2 if c8 >= 2 else 1
    return c8, CG, -(-c8 // CG)


def dw_wgrad_plan(N, H, W, C):
    """the launch of aldi_dwconv7_wgrad: quads, chunks with work, quads per chunk, chunk slots (a multiple of 8), pixel lanes, and the set of
    buffers (0: A, 1: B) on which a pixel lane's ping-pong loop ends"""
    c8, CG, ngrp = dw_groups(C)
    nquads = N * H * ((W + 3) // 4)
    chunks = min(1024 // (7 * ngrp) + 1, nquads // 64 + 1)
    ppb = -(-nquads // chunks)
    used = -(-nquads // ppb)
    slots = (used + 7) // 8 * 8
    npl = 256 // CG
    ends = set()
    for ch in range(used):
        q0, q1 = ch * ppb, min(nquads, (ch + 1) * ppb)
        for pl in range(npl):
            k = len(range(q0 + pl, q1, npl))
            if k:
                ends.add((k - 1) % 2)
    return dict(nquads=nquads, chunks=used, ppb=ppb, slots=slots, npl=npl, ends=ends, dead_groups=ngrp * CG - c8)


def dw_operands(N, H, W, C, seed):
    """integer x and g in [-4, 4], taps and bias in quarters with |w| <= 2: all bf16-representable"""
    g_ = torch.Generator().manual_seed(seed)
    return dict(x=ints(g_, (N, H, W, C), -4, 4), g=ints(g_, (N, H, W, C), -4, 4), wt=ints(g_, (7, 7, C), -8, 8) / 4, bias=ints(g_, (C,), -8, 8) / 4)


def dw_ref(x, wt, bias=None, flip=False):
    """y[n][h][w][c] = bias[c] + sum_{kh, kw} x[n][h + kh - 3][w + kw - 3][c] wt[kh][kw][c]; flip: the taps mirrored and no bias (the data gradient)"""
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 6, W + 6, C, dtype=x.dtype)
    xp[:, 3:H + 3, 3:W + 3] = x
    y = torch.zeros_like(x)
    for kh in range(7):
        for kw in range(7):
            y += xp[:, kh:kh + H, kw:kw + W] * (wt[6 - kh, 6 - kw] if flip else wt[kh, kw])
    return y if bias is None or flip else y + bias


def dw_wgrad_ref(x, g):
    """dw[kh][kw][c] = sum_{n, h, w} x[n][h + kh - 3][w + kw - 3][c] g[n][h][w][c]"""
    N, H, W, C = x.shape
    xp = torch.zeros(N, H + 6, W + 6, C, dtype=x.dtype)
    xp[:, 3:H + 3, 3:W + 3] = x
    return torch.stack([torch.stack([(xp[:, kh:kh + H, kw:kw + W] * g).sum((0, 1, 2)) for kw in range(7)]) for kh in range(7)])


def check_dw(ops):
    """the budget of the exact depthwise tests: products x w and g w are multiples of 1/4, x g integers -> the worst share in use"""
    assert on_lattice(ops["x"], 1) and on_lattice(ops["g"], 1) and on_lattice(ops["wt"], 0.25) and on_lattice(ops["bias"], 0.25)
    assert ops["x"].abs().max() <= 4 and ops["g"].abs().max() <= 4 and ops["wt"].abs().max() <= 2 and ops["bias"].abs().max() <= 2
    for t in ops.values():
        assert torch.equal(t, t.bfloat16().float())
    x, g, wt, bias = (ops[k].double().abs() for k in ("x", "g", "wt", "bias"))
    use = max(budget(dw_ref(x, wt, bias), 0.25), budget(dw_ref(g, wt, None, flip=True), 0.25), budget(dw_wgrad_ref(x, g), 1.0))
    assert use < 1.0, use
    return use


@functools.lru_cache(maxsize=None)
def dw_case(shape, C):
    """operands and the three fp64 references (forward, data gradient, weight gradient); computed once, never modified"""
    N, H, W = shape
    ops = dw_operands(N, H, W, C, 100 * H + W + C)
    check_dw(ops)
    x, g, wt, bias = (ops[k].double() for k in ("x", "g", "wt", "bias"))
    return ops, dict(y=dw_ref(x, wt, bias), y_nobias=dw_ref(x, wt), dgrad=dw_ref(g, wt, None, flip=True), wgrad=dw_wgrad_ref(x, g))


# ------------------------------------------------------------------------------------------------ layer-scale add
SA_ROWS, SA_ROWS_PER_SAMPLE = 333, 111
SA_KNOBS = (512, 10, 8, 1)                               # sab_blocks settings: the default and three that lengthen the row blocks


def sa_plan(rows, C, sab_blocks):
    """the launch of aldi_scale_add_backward: rows per block, blocks, and the set of row counts the four-rows-in-flight loop leaves to the tail loop"""
    c8, CG, ngrp = dw_groups(C)
    chunks = min(sab_blocks // ngrp + 1, rows // 64 + 1)
    rpb = -(-rows // chunks)
    blocks = -(-rows // rpb)
    nrl = 256 // CG
    left = set()
    for b in range(blocks):
        r0, r1 = b * rpb, min(rows, (b + 1) * rpb)
        for rl in range(nrl):
            k = len(range(r0 + rl, r1, nrl))
            left.add(k % 4)
    return dict(rpb=rpb, blocks=blocks, last=rows - (blocks - 1) * rpb, nrl=nrl, left=left)


def sa_operands(rows, C, seed, rows_per_sample=SA_ROWS_PER_SAMPLE):
    g_ = torch.Generator().manual_seed(seed)
    samples = -(-rows // rows_per_sample)
    return dict(x=ints(g_, (rows, C), -4, 4), y=ints(g_, (rows, C), -4, 4), g=ints(g_, (rows, C), -4, 4), gamma=choice(g_, (C,), (0.5, 1.0, 2.0)),
                scale=torch.tensor([0.0, 1.0, 2.0])[torch.arange(samples) % 3])


def sa_ref(x, y, g, gamma, scale=None, rows_per_sample=SA_ROWS_PER_SAMPLE):
    """out = x + s(r) gamma y, dy = s(r) gamma g, dgamma = sum_r s(r) g y"""
    s = torch.ones(x.shape[0], 1, dtype=x.dtype) if scale is None else scale[torch.arange(x.shape[0]) // rows_per_sample][:, None]
    return dict(out=x + s * gamma * y, dy=s * gamma * g, dgamma=(s * g * y).sum(0))


def check_sa(ops):
    assert all(on_lattice(ops[k], 1) and ops[k].abs().max() <= 4 for k in ("x", "y", "g")) and set(ops["gamma"].tolist()) <= {0.5, 1.0, 2.0}
    assert set(ops["scale"].tolist()) <= {0.0, 1.0, 2.0}
    x, y, g, gamma, scale = (ops[k].double().abs() for k in ("x", "y", "g", "gamma", "scale"))
    r = sa_ref(x, y, g, gamma, scale)
    use = max(budget(r["out"], 0.5), budget(r["dy"], 0.5), budget(r["dgamma"], 1.0))
    assert use < 1.0, use
    return use


@functools.lru_cache(maxsize=None)
def sa_case(C, with_scale):
    ops = sa_operands(SA_ROWS, C, 300 + C)
    check_sa(ops)
    d = {k: v.double() for k, v in ops.items()}
    return ops, sa_ref(d["x"], d["y"], d["g"], d["gamma"], d["scale"] if with_scale else None)

"""The token kernels of the ViTDet and ConvNeXt detectors (csrc/vit.hip, csrc/convnext.hip) one by one against the references of
token_kernel_refs.py (pinned on the CPU in test_token_kernels_cpu.py).

  * exact: LayerNorm backward (dgamma, dbeta always, dx for a power-of-two C), the constant / padded / clamped rows of LayerNorm forward, the row
    gather-add, patch extraction, identity resampling, add_pos / sum_batch, the 2 x 2 max pool, the depthwise 7 x 7 convolution with both gradients
    and the layer-scale add, on lattice operands: torch.equal with the explicit fp64 reference rounded once to the output dtype;
  * fp64-matched: LayerNorm forward, dx of LayerNorm backward for the other C, GELU, the scaled gather-add, the two resamplers and AdamW: per output
    tensor max|kernel - ref64| <= FACTOR * max|ref32 - ref64| + 4 * 2^-24 * max|ref64| (+ half a bf16 ulp of each reference element for a bf16
    output), ref32 / ref64 = the same function in fp32 / fp64 on the CPU.  GELU is judged per element (R.gelu_allowed).

The measured ratios are in the table below FACTOR.  Every check prints its figures before it asserts (pytest -s)."""
import pytest
import torch

import token_kernel_refs as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
# Measured on an MI355X: err_kernel / err_ref32, the largest over the cases of each test (`-`: both errors are zero; for a bf16 output the error is
# what remains beyond half a bf16 ulp of the reference).  No entry needed more than FACTOR, so the bound is FACTOR everywhere.
#
#   layernorm forward, fp32 (5 C x 4 kinds of row)    randn: y 1.41 mean 1.80 rstd 1.33    randn + 30: y 1.00 mean 1.00 rstd 1.82
#                                                     1e-3 randn + 100: y 1.19 mean 1.19 rstd 1.46    1e4 outlier: y 1.75 mean 1.24 rstd 1.56
#   layernorm forward, bf16 (11 forms)                randn: y 0.04 mean 2.00 rstd 1.00    randn + 30: y 0.44 mean 1.00 rstd 2.83
#                                                     1e-3 randn + 100 (constant rows in bf16): y -  mean -  rstd 0.02    1e4 outlier: y 0.00 mean 1.89 rstd 1.68
#   layernorm forward through a row map               y fp32 1.00, bf16 0.16
#   layernorm backward, dx where C is no power of two fp32 1.00 (C = 100, 1028)   bf16 0.40 (C = 100, 520, 1028, 1032); dgamma, dbeta and every other dx: exact
#   rows_add, scale 1 / 0.9                           out fp32 1.00, bf16 0.39
#   linear_resize (9 shapes)                          out 1.34   dtable 1.01
#   bicubic_resize (10 shapes, 5 non-square sources)  out 1.21   dgrid 1.53
#   adamw (steps 1, 2, 3, 1000, 100000)               p 1.00   m 1.00   v 1.00
#
# GELU is judged per element against 1.5e-7 max(1, |x|) (|g|) + the tolerance of fp32 F.gelu in the element's binade (+ half a bf16 ulp); measured:
#
#   fp32 forward    worst err / allowed 0.24 (x = -0.738)   worst err 4.17e-7 at x = 3.172 (the CPU transcription of the formula: 3.9e-7 there)
#   fp32 backward   worst err / allowed 0.13 (x = -0.75)    worst err 1.21e-6 at x = 0.0012, |g| = 4.2
#   bf16 forward    worst err / allowed 0.008 beyond half an ulp; 113 of the 33356 outputs differ from the rounded truth, 51 of them by more than one
#                   ulp (at most 5), all at x <= -6.75 where |gelu(x)| <= 5e-11: the relative error of the Abramowitz-Stegun form grows in the
#                   far tail, its absolute error does not.  The 8-wide form and both 4-wide forms give the same figures.
#   bf16 backward   every output is the rounded truth
#
# No test of this file has failed on the kernels as they are: csrc/vit.hip and csrc/convnext.hip are unchanged.


@pytest.fixture(autouse=True)
def reset_tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _lib():
    from aldi_amd import _lib as L
    from aldi_amd import vit_ops as V
    from aldi_amd.ops import _p, dtype_code, stream_ptr
    return L, V, _p, dtype_code, stream_ptr


def dev(t, dtype=None, off=0, fill=None):
    """t on the device in `dtype`; off: as a view that starts `off` elements into its (512-B aligned) buffer; fill: the values replaced by `fill`"""
    if t is None:
        return None
    dtype = dtype or t.dtype
    buf = torch.empty(t.numel() + off, dtype=dtype, device="cuda")
    v = buf[off:].view(t.shape)
    if fill is None:
        v.copy_(t.to(dtype))
    else:
        v.fill_(fill)
    assert v.data_ptr() % 16 == (off * v.element_size()) % 16
    return v


NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16"}


class Check:
    """collects the fp64-matched comparisons of one test: prints every figure, fails at the end with all that missed"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def __call__(self, name, got, r32, r64, factor=FACTOR):
        lowp = got.dtype == torch.bfloat16
        got = got.detach().cpu().double().reshape(r64.shape)
        err = (got - r64).abs()
        if lowp:
            err = (err - R.bf16_half_ulp(r64)).clamp(min=0)
        ek, er = err.max().item(), (r32.double() - r64).abs().max().item()
        tol = R.tolerance(r32, r64, factor)
        finite = bool(torch.isfinite(got).all())
        print(f"RATIO {self.what:<52} {name:<7} err_kernel {ek:.3e} err_ref32 {er:.3e} ratio {ek / er if er else float('nan'):8.3f} tol {tol:.3e} max|ref| {r64.abs().max().item():.3e}")
        if not (finite and ek <= tol):
            self.bad.append((name, ek, er, tol))

    def done(self):
        assert not self.bad, (self.what, self.bad)


def _equal(got, ref64, what):
    """got == the fp64 reference rounded once to got's dtype, and nothing is NaN"""
    ref = R.round_to(ref64, got.dtype).float()
    g = got.detach().cpu().float().reshape(ref.shape)
    bad = g != ref
    assert not bad.any() and not torch.isnan(g).any(), (what, int(bad.sum()), int(torch.isnan(g).sum()), (g - ref).abs().nan_to_num(9e9).max().item(),
                                                         bad.nonzero()[:4].tolist())


# ================================================================================================ 1. LayerNorm backward
LN_BWD_PARAMS = ([(torch.bfloat16, C, 0) for C in R.LN_C_BF16_WIDE + R.LN_C_BF16_NARROW] + [(torch.bfloat16, 256, 4)]
                 + [(torch.float32, C, 0) for C in R.LN_C_F32])
# (rows, res, mask, ln_bwd_blocks / ln_bwd_blocks_narrow or None for the default, row map)
LN_BWD_RUNS = [(1, True, True, None, False), (3, False, False, None, False), (333, False, False, None, False), (333, True, False, None, False),
               (333, False, True, None, False), (333, True, True, None, False), (333, True, True, 4, False), (333, False, False, 4, False),
               (1025, True, True, None, False), (0, True, True, None, True), (0, False, False, None, True)]


@pytest.mark.parametrize("dtype,C,off", LN_BWD_PARAMS, ids=lambda v: NAMES.get(v, str(v)))
def test_layernorm_backward_on_lattice_operands(dtype, C, off):
    """dgamma and dbeta equal the reference bit for bit for every C, dx for a power-of-two C (fp64-matched otherwise); dx starts as NaN, so every
    source row has to be written; off = 4: the operands start 8 bytes into a 16-B aligned buffer, which forces the 4-wide form at C = 256"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    c = Check(f"ln_bwd {NAMES[dtype]} C {C}")
    for rows, res, mask, knob, use_map in LN_BWD_RUNS:
        ops, r64, r32, _ = R.ln_bwd_case(rows, C, res, mask, use_map)
        L.reset_tuning()
        if knob is not None:
            L.set_tuning("ln_bwd_blocks", knob)
            L.set_tuning("ln_bwd_blocks_narrow", knob)
        g, x, rs_, mk = dev(ops["g"], dtype, off), dev(ops["x"], dtype, off), dev(ops["res"] if res else None, dtype, off), dev(ops["mask"] if mask else None, dtype, off)
        dx = dev(ops["x"], dtype, off, fill=float("nan"))
        gamma, mean, rstd = ops["gamma"].cuda(), ops["mean"].cuda(), ops["rstd"].cuda()
        row_map = ops["row_map"].cuda() if use_map else None
        dgamma, dbeta = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        out = V.layernorm_backward(g, x, gamma, mean, rstd, dgamma, dbeta, row_map=row_map, res=rs_, mask=mk, out=dx)
        torch.cuda.synchronize()
        what = (NAMES[dtype], C, off, rows, res, mask, knob, use_map)
        assert out.data_ptr() == dx.data_ptr()
        _equal(dgamma, r64["dgamma"], what + ("dgamma",))
        _equal(dbeta, r64["dbeta"], what + ("dbeta",))
        assert not torch.isnan(dx.float()).any(), what + ("a source row was not written",)
        if R.is_pow2(C):
            _equal(dx, r64["dx"], what + ("dx",))
        else:
            c.what = f"ln_bwd {NAMES[dtype]} C {C} rows {rows} res {int(res)} mask {int(mask)} knob {knob} map {int(use_map)}"
            c("dx", dx, r32["dx"], r64["dx"])
    c.done()


# ================================================================================================ 2. LayerNorm forward
LN_FWD_PARAMS = LN_BWD_PARAMS


@pytest.mark.parametrize("dtype,C,off", LN_FWD_PARAMS, ids=lambda v: NAMES.get(v, str(v)))
def test_layernorm_forward_against_fp64(dtype, C, off):
    """y, mean and rstd on rows of randn, randn + 30, 1e-3 randn + 100 and a single 1e4 outlier, each kind judged on its own (fp32 itself loses
    most of the third kind, whose tolerance would swamp the others)"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    x, gamma, beta = R.ln_fwd_operands(C, 11 + C, dtype)
    r32, r64 = R.both(R.ln_fwd_ref, x, gamma, beta)
    y, mean, rstd = V.layernorm_forward(dev(x, dtype, off), gamma.cuda(), beta.cuda(), eps=R.LN_EPS)
    torch.cuda.synchronize()
    c = Check("")
    n = x.shape[0] // 4
    for k, kind in enumerate(R.LN_FWD_KINDS):
        c.what = f"ln_fwd {NAMES[dtype]} C {C} off {off} {kind}"
        s = slice(k * n, (k + 1) * n)
        c("y", y[s], r32["y"][s], r64["y"][s]); c("mean", mean[s], r32["mean"][s], r64["mean"][s]); c("rstd", rstd[s], r32["rstd"][s], r64["rstd"][s])
    c.done()


@pytest.mark.parametrize("dtype,C,off", LN_FWD_PARAMS, ids=lambda v: NAMES.get(v, str(v)))
def test_layernorm_forward_exact_rows(dtype, C, off):
    """a constant integer row gives y == beta, mean == the value and rstd within 2 fp32 ulps of eps^-1/2; a row mapped to -1 is all zero with
    mean == rstd == 0; relu=True is clamp_min(0) of the relu=False output, bit for bit"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    g_ = torch.Generator().manual_seed(C)
    values = torch.tensor([0.0, 1.0, -3.0, 7.0, 100.0, -128.0])
    x = torch.cat([values[:, None].expand(6, C), torch.randn(5, C, generator=g_).to(dtype).float()]).contiguous()
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g_), torch.randn(C, generator=g_)
    row_map = torch.tensor([0, 1, -1, 2, 3, 4, 5, -1, 6, 7, 10, 9, 8, -1, 6], dtype=torch.int32)
    xd, gd, bd, md = dev(x, dtype, off), gamma.cuda(), beta.cuda(), row_map.cuda()
    y, mean, rstd = V.layernorm_forward(xd, gd, bd, eps=R.LN_EPS, row_map=md)
    yr, mean_r, rstd_r = V.layernorm_forward(xd, gd, bd, eps=R.LN_EPS, row_map=md, relu=True)
    torch.cuda.synchronize()
    y, mean, rstd, yr = y.cpu(), mean.cpu(), rstd.cpu(), yr.cpu()
    const = (row_map >= 0) & (row_map < 6)
    assert torch.equal(y[const], beta.to(dtype).expand(int(const.sum()), C))
    assert torch.equal(mean[const], values[row_map[const].long()])
    target = 1 / torch.tensor(R.f32(R.LN_EPS), dtype=torch.float64).sqrt()
    assert ((rstd[const].double() - target).abs() <= 2 * 2.0 ** -14).all(), rstd[const]                # an ulp of 1000 is 2^-14
    pad = row_map < 0
    assert (y[pad].float() == 0).all() and (mean[pad] == 0).all() and (rstd[pad] == 0).all()
    assert torch.equal(yr, y.clamp_min(0)) and torch.equal(mean_r.cpu(), mean) and torch.equal(rstd_r.cpu(), rstd)
    assert (yr == 0).any() and (yr > 0).any()
    r32, r64 = R.both(R.ln_fwd_ref, x, gamma, beta, row_map=row_map)
    c = Check(f"ln_fwd {NAMES[dtype]} C {C} off {off} mapped")
    rnd = row_map >= 6
    c("y", y[rnd], r32["y"][rnd], r64["y"][rnd])
    c.done()


# ================================================================================================ 3. GELU
@pytest.mark.parametrize("form", ["bf16 8-wide", "bf16 4-wide n % 8 == 4", "bf16 4-wide unaligned", "fp32"])
def test_gelu_on_every_bf16_value(form):
    """forward and backward on all finite bf16 values in [-10, 10], +-20, +-100, +-1e4 and the largest finite bf16 (fp32: plus a grid of 2e5
    points): per element within 1.5e-7 max(1, |x|) (|g|) + the fp32 F.gelu yardstick's tolerance (+ half a bf16 ulp), never NaN, and exactly
    x or a zero of the right sign (g or a zero) from 1e4 on"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    dtype = torch.float32 if form == "fp32" else torch.bfloat16
    x, g = R.gelu_inputs(200000 if form == "fp32" else 0)
    off = 0
    if form == "bf16 4-wide n % 8 == 4":
        x, g = torch.cat([x, torch.full((4,), -0.5)]), torch.cat([g, torch.ones(4)])
    elif form == "bf16 4-wide unaligned":
        off = 4
    assert x.numel() % 8 == (4 if "n % 8" in form else 0)
    xd, gd = dev(x, dtype, off), dev(g, dtype, off)
    out_f, out_b = dev(x, dtype, off, fill=float("nan")), dev(x, dtype, off, fill=float("nan"))
    L.call("aldi_gelu", _p(xd), None, _p(out_f), x.numel(), dtype_code(dtype), stream_ptr())
    L.call("aldi_gelu", _p(xd), _p(gd), _p(out_b), x.numel(), dtype_code(dtype), stream_ptr())
    torch.cuda.synchronize()
    bad = []
    for name, got, gg in (("forward", out_f, None), ("backward", out_b, g)):
        got = got.cpu().float()
        truth, allowed, banded = R.gelu_allowed(x, gg, lowp=dtype == torch.bfloat16)
        err = (got.double() - truth).abs()
        half = R.bf16_half_ulp(truth) if dtype == torch.bfloat16 else torch.zeros_like(truth)
        excess = (err - half).clamp(min=0)                             # err <= allowed  <=>  excess <= allowed - half
        ratio = torch.where(banded, excess / (allowed - half), torch.zeros_like(err))
        i, j = int(ratio.argmax()), int(torch.where(banded, excess, torch.zeros_like(excess)).argmax())
        print(f"\nGELU {form:<24} {name:<8} worst err / allowed {ratio[i].item():.3f} at x = {x[i].item():.6g} (err {excess[i].item():.3e});   worst err "
              f"{excess[j].item():.3e} at x = {x[j].item():.6g}" + ("   (both beyond half a bf16 ulp of the truth)" if dtype == torch.bfloat16 else ""))
        if dtype == torch.bfloat16:
            ulps = torch.where(banded, (got.double() - truth.float().bfloat16().double()).abs() / (2 * half), torch.zeros_like(err))
            off1 = ulps > 1
            print(f"GELU {form:<24} {name:<8} bf16 outputs: {int((ulps > 0).sum())} of {int(banded.sum())} differ from the rounded truth, {int(off1.sum())} by more than one ulp"
                  + (f" (at most {ulps.max().item():.1f}, all of them at x <= {x[off1].max().item():.6g}, where |truth| <= {truth[off1].abs().max().item():.2e})" if off1.any() else ""))
        if torch.isnan(got).any() or not (ratio <= 1).all():
            bad.append((name, int(torch.isnan(got).sum()), ratio.max().item()))
        far = ~banded
        assert far.sum() == 4
        xf, gf = x[far], got[far]
        if gg is None:
            want = torch.where(xf > 0, xf, -torch.zeros_like(xf))
            assert R.same_bits(gf, want), (name, xf, gf)
        else:
            assert torch.equal(gf, torch.where(xf > 0, gg[far], torch.zeros_like(xf))), (name, xf, gf)
    assert not bad, (form, bad)


# ================================================================================================ 4. the row gather-add
@pytest.mark.parametrize("C,off", [(64, 0), (100, 0), (64, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_rows_add(dtype, C, off):
    L, V, _p, dtype_code, stream_ptr = _lib()
    g_ = torch.Generator().manual_seed(C + off)
    rows, n_src, rps = 40, 25, 7                                       # 7 rows per sample: no divisor of the 256 threads of a block
    a, b_same, b_src = R.ints(g_, (rows, C), -4, 4), R.ints(g_, (rows, C), -4, 4), R.ints(g_, (n_src, C), -4, 4)
    m = torch.randint(-1, n_src, (rows,), generator=g_, dtype=torch.int32)
    m[3], m[rows - 1] = -1, -1
    scale = torch.tensor([0.0, 1.0, 2.0, 1.0, 0.0, 2.0])
    ad, bd, bs = dev(a, dtype, off), dev(b_same, dtype, off), dev(b_src, dtype, off)

    def run(a_, b_, map_, scale_, rps_):
        out = dev(a, dtype, off, fill=float("nan"))
        V.rows_add(a_, b_, rows=rows, row_map=None if map_ is None else map_.cuda(), scale=None if scale_ is None else scale_.cuda(), rows_per_sample=rps_, out=out)
        torch.cuda.synchronize()
        return out

    _equal(run(None, bd, None, None, 1), R.rows_add_ref(None, b_same.double()), "a = None")
    _equal(run(ad, bs, m, None, 1), R.rows_add_ref(a.double(), b_src.double(), m), "map")
    _equal(run(ad, bd, None, scale, rps), R.rows_add_ref(a.double(), b_same.double(), None, scale.double(), rps), "scale")
    _equal(run(ad, bs, m, scale, rps), R.rows_add_ref(a.double(), b_src.double(), m, scale.double(), rps), "map + scale")
    _equal(run(None, bs, m, scale, rps), R.rows_add_ref(None, b_src.double(), m, scale.double(), rps), "a = None, map + scale")
    # drop path: scale 1 / 0.9 on random rows
    ar, br = torch.randn(rows, C, generator=g_).to(dtype).float(), torch.randn(rows, C, generator=g_).to(dtype).float()
    sc = torch.tensor([0.0, 1 / 0.9, 1 / 0.9, 0.0, 1 / 0.9, 1 / 0.9])
    r32, r64 = R.both(R.rows_add_ref, ar, br, None, sc, rps)
    out = dev(a, dtype, off, fill=float("nan"))
    V.rows_add(dev(ar, dtype, off), dev(br, dtype, off), rows=rows, scale=sc.cuda(), rows_per_sample=rps, out=out)
    c = Check(f"rows_add {NAMES[dtype]} C {C} off {off} scale 1/0.9")
    c("out", out, r32, r64)
    c.done()


# ================================================================================================ 5. patch extraction
@pytest.mark.parametrize("P", [4, 16])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_patchify_equals_the_fp32_expression(dtype, P):
    """((float) u8 - mean) * (1.f / std), bit for bit; the staging bytes outside each image are 255 and must come out as exact zeros"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    img, hw = R.patchify_operands(P, 4 + P)
    ref = R.patchify_ref(img, hw, P)
    got = V.patchify(img.cuda(), hw.flatten().cuda(), P, R.PIXEL_MEAN, R.PIXEL_STD, dtype)
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(got, ref.to(dtype))
    outside = torch.ones(3, 3, 64, 96)
    for n, (h, w) in enumerate(hw.tolist()):
        outside[n, :, :h, :w] = 0
    o = outside.view(3, 3, 64 // P, P, 96 // P, P).permute(0, 2, 4, 1, 3, 5).reshape(got.shape).bool()
    assert o.sum() > 1000 and (got[o].float() == 0).all() and not torch.signbit(got[o].float()).any()


# ================================================================================================ 6. the resamplers
@pytest.mark.parametrize("L0,L1", R.LINEAR_CASES)
def test_linear_resize(L0, L1):
    L, V, _p, dtype_code, stream_ptr = _lib()
    C = 70                                                             # more channels than the 64 threads of a block
    g_ = torch.Generator().manual_seed(L0 * 100 + L1)
    t, g = torch.randn(L0, C, generator=g_), torch.randn(L1, C, generator=g_)
    out = V.linear_resize(t.cuda(), L1)
    dt = torch.zeros(L0, C, device="cuda")
    V.linear_resize_backward(g.cuda(), dt)
    torch.cuda.synchronize()
    if L0 == L1:
        assert torch.equal(out.cpu(), t) and torch.equal(dt.cpu(), g)
    c = Check(f"linear_resize {L0} -> {L1}")
    c("out", out, *R.both(R.linear_ref, t, L1=L1))
    c("dtable", dt, *R.both(R.linear_ref, g, L1=L1, backward_into=L0))
    c.done()


@pytest.mark.parametrize("case", R.BICUBIC_CASES, ids=str)
def test_bicubic_resize(case):
    L, V, _p, dtype_code, stream_ptr = _lib()
    S0h, S0w, gh, gw = case
    C = 260                                                            # more channels than the 256 threads of a block
    g_ = torch.Generator().manual_seed(sum(case))
    t, g = torch.randn(S0h, S0w, C, generator=g_), torch.randn(gh, gw, C, generator=g_)
    out = V.bicubic_resize(t.cuda(), gh, gw)
    dt = torch.zeros(S0h, S0w, C, device="cuda")
    V.bicubic_resize_backward(g.cuda(), dt)
    torch.cuda.synchronize()
    if (S0h, S0w) == (gh, gw):
        assert torch.equal(out.cpu(), t) and torch.equal(dt.cpu(), g)
    c = Check(f"bicubic_resize {case}")
    c("out", out, *R.both(R.bicubic_ref, t, gh=gh, gw=gw))
    c("dgrid", dt, *R.both(R.bicubic_ref, g, gh=gh, gw=gw, backward_into=(S0h, S0w)))
    c.done()


# ================================================================================================ 7. add_pos, sum_batch
@pytest.mark.parametrize("T,C", [(1, 4), (35, 36)])                  # TC = 4 and TC = 1260, no multiple of 1024
@pytest.mark.parametrize("N", [1, 33])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_add_pos_and_sum_batch(dtype, N, T, C):
    L, V, _p, dtype_code, stream_ptr = _lib()
    g_ = torch.Generator().manual_seed(N + T)
    x, pos = R.ints(g_, (N, T, C), -4, 4), R.ints(g_, (T, C), -4, 4)
    xd = dev(x, dtype)
    y = V.add_pos(xd, pos.cuda(), N)
    s = V.sum_batch(xd, N)
    torch.cuda.synchronize()
    _equal(y, x.double() + pos.double(), "add_pos")
    assert s.dtype == torch.float32
    _equal(s.view(T, C), x.double().sum(0), "sum_batch")


# ================================================================================================ 8. the 2 x 2 max pool
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_maxpool2_ties_zeros_infinities_and_nans(dtype):
    L, V, _p, dtype_code, stream_ptr = _lib()
    x, g = R.maxpool_operands()
    ty, ttap = R.maxpool_torch(x)
    y, idx = V.maxpool2(dev(x, dtype))
    dx = V.maxpool2_backward(dev(g, dtype), idx, x.shape[1], x.shape[2])
    torch.cuda.synchronize()
    assert R.same_bits(y.cpu(), ty), (y.cpu().float() - ty).abs().nan_to_num(0).max()
    assert torch.equal(idx.cpu(), ttap), (idx.cpu() != ttap).nonzero()[:8].tolist()
    assert torch.equal(dx.cpu().float(), R.maxpool_bwd_ref(g, ttap, x.shape[1], x.shape[2]))


# ================================================================================================ 9. AdamW
@pytest.mark.parametrize("grad_scale", [1.0, 0.3])
@pytest.mark.parametrize("n", [1, 1000])
def test_adamw_steps_against_fp64(n, grad_scale):
    """p, m and v after each of the steps 1, 2, 3 (from zero moments) and after step 1000 and step 100000 (moments pre-set); the truth of every step
    is the fp64 reference on the kernel's own state before it and on the fp32-rounded hyper-parameters; p_compute == p.bfloat16()"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    h = R.adamw_hyper(grad_scale)
    c = Check("")
    for first, late, count in ((1, False, 3), (1000, True, 1), (100000, True, 1)):
        p, g, m, v = R.adamw_operands(n, first + n, late)
        assert g[0] == 0 and v[0] == 0
        pd, gd, md, vd = p.cuda(), g.cuda(), m.cuda(), v.cuda()
        pc = torch.full((n,), float("nan"), dtype=torch.bfloat16, device="cuda")
        for step in range(first, first + count):
            state = [t.cpu() for t in (pd, gd, md, vd)]
            r32, r64 = R.both(R.adamw_ref, *state, step=step, **h)
            V.adamw_step(pd, gd, md, vd, pc, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"], step=step, grad_scale=h["grad_scale"])
            torch.cuda.synchronize()
            c.what = f"adamw n {n} grad_scale {grad_scale} step {step}"
            c("p", pd, r32["p"], r64["p"]); c("m", md, r32["m"], r64["m"]); c("v", vd, r32["v"], r64["v"])
            assert torch.equal(pc, pd.bfloat16())
    c.done()


# ================================================================================================ 10. depthwise 7 x 7
@pytest.mark.parametrize("C", R.DW_CHANNELS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_depthwise_forward_and_both_gradients_on_lattice_operands(dtype, C):
    """aldi_dwconv7 (with and without bias), its flipped form on the gradient and aldi_dwconv7_wgrad == fp64 conv2d(groups=C) and its autograd, bit
    for bit; the outputs start as NaN"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    for shape in R.DW_SHAPES:
        N, H, W = shape
        ops, ref = R.dw_case(shape, C)
        x, g, wt, bias = dev(ops["x"], dtype), dev(ops["g"], dtype), dev(ops["wt"], dtype), ops["bias"].cuda()
        what = (NAMES[dtype], C, shape)
        for name, src, b, flip in (("y", x, bias, 0), ("y_nobias", x, None, 0), ("dgrad", g, None, 1), ("dgrad", g, bias, 1)):
            y = dev(ops["x"], dtype, fill=float("nan"))
            L.call("aldi_dwconv7", _p(src), _p(wt), _p(b), _p(y), N, H, W, C, flip, dtype_code(dtype), stream_ptr())
            torch.cuda.synchronize()
            _equal(y, ref[name], what + (name, b is not None))
        dw = torch.zeros(7, 7, C, device="cuda")
        V.dwconv7_wgrad(x, g, dw)
        V.dwconv7_wgrad(x, g, dw)                                      # accumulates
        torch.cuda.synchronize()
        _equal(dw, 2 * ref["wgrad"], what + ("wgrad",))


# ================================================================================================ 11. layer-scale add
@pytest.mark.parametrize("C", R.DW_CHANNELS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: NAMES[v])
def test_scale_add_forward_backward_on_lattice_operands(dtype, C):
    """out, dy and dgamma == the reference, bit for bit, under sab_blocks settings that give the row blocks a tail and leave the four-rows-in-flight
    loop 0, 1, 2 and 3 rows (asserted on the launch arithmetic in test_token_kernels_cpu.py)"""
    L, V, _p, dtype_code, stream_ptr = _lib()
    for with_scale in (True, False):
        ops, ref = R.sa_case(C, with_scale)
        x, y, g = dev(ops["x"], dtype), dev(ops["y"], dtype), dev(ops["g"], dtype)
        gamma, scale = ops["gamma"].cuda(), ops["scale"].cuda() if with_scale else None
        for knob in R.SA_KNOBS:
            L.reset_tuning()
            L.set_tuning("sab_blocks", knob)
            out = V.scale_add(x, y, gamma, scale, R.SA_ROWS_PER_SAMPLE)
            dgamma = torch.zeros(C, device="cuda")
            dy = V.scale_add_backward(g, y, gamma, scale, dgamma, R.SA_ROWS_PER_SAMPLE)
            torch.cuda.synchronize()
            what = (NAMES[dtype], C, with_scale, knob)
            _equal(out, ref["out"], what + ("out",)); _equal(dy, ref["dy"], what + ("dy",)); _equal(dgamma, ref["dgamma"], what + ("dgamma",))

"""The references of tests/token_kernel_refs.py pinned without a GPU: every explicit reference equals an independent torch function in fp64
(F.layer_norm and autograd, F.gelu, F.conv2d(groups=C), F.interpolate, F.unfold, F.max_pool2d(return_indices=True), torch.optim.AdamW on a double
parameter), every lattice construction stays inside its bit budget, and the shapes and knobs of the GPU tests reach the launch geometry
(row tails, empty chunk slots, ping-pong parity, rows left for the tail loop) they are meant to reach."""

import pytest
import torch
import torch.nn.functional as F

import token_kernel_refs as R

ALL_LN_C = sorted(set(R.LN_C_BF16_WIDE + R.LN_C_BF16_NARROW + R.LN_C_F32 + (256,)))


def _close(a, b, rtol=1e-12):
    return (a - b).abs().max().item() <= rtol * max(b.abs().max().item(), 1.0)


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("use_map", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [4, 100, 520])
def test_layernorm_references_equal_torch_autograd(C, relu, use_map):
    """ln_fwd_ref == F.layer_norm (window-partitioned, clamped); ln_bwd_ref on its statistics, with the ReLU mask and a residual == autograd"""
    g_ = torch.Generator().manual_seed(C)
    row_map = R.partition_map(*R.LN_MAP) if use_map else None
    n_src = 60 if use_map else 37
    x = (torch.randn(n_src, C, generator=g_, dtype=torch.float64) * 2 + 0.5).requires_grad_(True)
    gamma = (1 + 0.5 * torch.randn(C, generator=g_, dtype=torch.float64)).requires_grad_(True)
    beta = torch.randn(C, generator=g_, dtype=torch.float64).requires_grad_(True)
    res = torch.randn(n_src, C, generator=g_, dtype=torch.float64)
    y = F.layer_norm(x, (C,), gamma, beta, R.f32(R.LN_EPS))
    if use_map:
        y = y[row_map.clamp(min=0).long()] * (row_map >= 0)[:, None]
    if relu:
        y = y.clamp_min(0)
    got = R.ln_fwd_ref(x.detach(), gamma.detach(), beta.detach(), row_map=row_map, relu=relu)
    assert _close(got["y"], y.detach())
    if use_map:
        pad = row_map < 0
        assert pad.sum() == 68 and (got["y"][pad] == 0).all() and (got["mean"][pad] == 0).all() and (got["rstd"][pad] == 0).all()
    g = torch.randn(y.shape, generator=g_, dtype=torch.float64)
    y.backward(g)
    mask = (y.detach() > 0).double() if relu else None
    bw = R.ln_bwd_ref(g, x.detach(), gamma.detach(), got["mean"], got["rstd"], res, mask, row_map)
    assert _close(bw["dx"], x.grad + res) and _close(bw["dgamma"], gamma.grad) and _close(bw["dbeta"], beta.grad)


@pytest.mark.parametrize("C", ALL_LN_C)
def test_layernorm_backward_lattice_stays_inside_its_budget(C):
    worst = 0.0
    for rows in R.LN_ROWS:
        ops, r64, r32, bits = R.ln_bwd_case(rows, C, True, True)
        worst = max(worst, bits)
        for k in ("dgamma", "dbeta"):                      # the order of a sum and the width of the format do not matter
            assert torch.equal(r32[k].double(), r64[k])
        if R.is_pow2(C):
            assert torch.equal(r32["dx"].double(), r64["dx"])
            R.round_to(r64["dx"], torch.bfloat16)
        assert (r64["dgamma"] != 0).any() and (r64["dbeta"] != 0).any() or rows * C < 16
    print(f"LN backward lattice C {C}: the widest intermediate needs {worst:.1f} bits")
    assert worst < 24
    if C == 2048:
        assert 14 <= worst <= 20.1                        # the construction allows (2 + 2 + 8 * 16) * 2 C: 20 bits; these operands use 16


def test_layernorm_backward_lattice_with_a_row_map():
    ops, r64, r32, bits = R.ln_bwd_case(0, 256, True, True, True)
    m = ops["row_map"]
    assert m.numel() == 128 and (m < 0).sum() == 68 and sorted(m[m >= 0].tolist()) == list(range(60))
    assert torch.isnan(ops["mean"][m < 0]).all() and (ops["g"][m < 0] == 1).all()
    assert torch.equal(r32["dx"].double(), r64["dx"]) and torch.equal(r32["dgamma"].double(), r64["dgamma"]) and not torch.isnan(r64["dx"]).any()
    # the gradients behind a zero of the mask do not reach dgamma / dbeta
    _, plain, _, _ = R.ln_bwd_case(333, 64, False, False)
    _, masked, _, _ = R.ln_bwd_case(333, 64, False, True)
    assert not torch.equal(plain["dbeta"], masked["dbeta"]) and not torch.equal(plain["dgamma"], masked["dgamma"])


def test_layernorm_backward_row_blocks():
    """the default knobs give whole blocks of 32 rows and a short last one; 4 blocks give 84 rows per block and a last block of 81, which the four
    waves leave after 21, 20, 20, 20 rows: the prefetch loop ends on either parity"""
    assert R.ln_bwd_plan(333, 512) == (32, 11, 13) and R.ln_bwd_plan(1025, 1024) == (32, 33, 1) and R.ln_bwd_plan(1, 512) == (32, 1, 1)
    assert R.ln_bwd_plan(333, 4) == (84, 4, 81)
    assert {len(range(w, 84, 4)) % 2 for w in range(4)} == {1} and {len(range(w, 81, 4)) % 2 for w in range(4)} == {0, 1}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_forward_operands(dtype):
    x, gamma, beta = R.ln_fwd_operands(64, 3, dtype)
    assert torch.equal(x, x.to(dtype).float()) and x.shape == (20, 64)
    assert (x[15:].abs() > 5000).sum(1).tolist() == [1] * 5 and 29 < x[5:10].mean() < 31 and 99 < x[10:15].mean() < 101
    r32, r64 = R.both(R.ln_fwd_ref, x, gamma, beta)
    tol = [R.tolerance(r32["y"][5 * k:5 * k + 5], r64["y"][5 * k:5 * k + 5]) for k in range(4)]
    print("LN forward: the tolerance of y per kind of row", dict(zip(R.LN_FWD_KINDS, tol)))
    assert tol[0] < 2e-5 and tol[1] < 1e-3            # fp32 itself loses the rows of 1e-3 randn + 100: the kinds are judged one by one


# ------------------------------------------------------------------------------------------------ GELU
def test_gelu_reference_equals_torch_and_covers_every_bf16_value():
    x, g = R.gelu_inputs()
    assert x.numel() % 8 == 0 and torch.equal(x, x.bfloat16().float()) and torch.equal(g, g.bfloat16().float()) and (g != 0).all()
    v = R.bf16_values()
    assert v.numel() == 2 * (1 + 127 + (130 - 1) * 128 + 33)          # per sign: zero, subnormals, binades 2^-126 .. 2^2 in full, [8, 10] = 33 values
    assert (v == 0).sum() == 2 and torch.signbit(v[v == 0]).sum() == 1 and v.max() == 10 and v.min() == -10
    assert {20.0, -100.0}.issubset(set(x.tolist())) and x.abs().max() == torch.finfo(torch.bfloat16).max and (x.abs() > R.GELU_FAR).sum() == 4
    x64, g64 = x.double(), g.double()
    near = x64.abs() <= 100
    y, dy = R.gelu_ref(x64), R.gelu_ref(x64, g64)
    ty, tdy = R.gelu_torch(x64), R.gelu_torch(x64, g64)
    # F.gelu is 0.5 x (1 + erf): absolute error 1e-16 |x| in the negative tail, where the erfc form keeps its relative precision
    assert ((y - ty).abs()[near] <= 4e-16 * x64.abs().clamp(min=1)[near]).all()
    assert ((dy - tdy).abs()[near] <= 4e-16 * (x64.abs().clamp(min=1) * g64.abs())[near]).all()
    far = x64.abs() > R.GELU_FAR
    assert torch.equal(y[far], torch.where(x64[far] > 0, x64[far], -torch.zeros_like(x64[far]))) or ((y[far & (x64 < 0)]).abs() < 1e-300).all()
    assert torch.isfinite(y).all() and torch.isfinite(dy).all()
    assert y[x64 == -5.0].item() == pytest.approx(-5.0 * 2.8665157187919333e-07, rel=1e-12)       # Phi(-5)


def test_gelu_allowed_error_holds_the_kernels_formula():
    """the bound per element is that of the element's own binade, and the fp32 transcription of the kernel's formula on the CPU stays within it"""
    x, g = R.gelu_inputs(2000)
    truth, allowed, banded = R.gelu_allowed(x, None, lowp=False)
    i = int((x == -5.0).nonzero()[0])
    j = int((x - 3.05).abs().argmin())
    print(f"GELU forward: allowed at x = -5: {allowed[i].item():.3e} (truth {truth[i].item():.3e}), at x = {x[j].item():.4f}: {allowed[j].item():.3e}")
    assert R.GELU_AS_BOUND * 5 <= allowed[i] < 1e-5 and allowed[j] < 1e-5      # fp32 F.gelu itself is 8e-7 off in (2, 4]
    assert banded.sum() == x.numel() - 4
    z = x.abs() * 0.70710678118654752
    t = 1 / (0.3275911 * z + 1)
    e = torch.exp(-z * z)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592)
    half = 0.5 * p * t * e
    cdf = torch.where(x >= 0, 1 - half, half)
    err = ((x * cdf).double() - truth).abs()
    print(f"GELU transcription on the CPU: worst err / allowed {(err / allowed)[banded].max().item():.3f}, worst err {err[banded].max().item():.3e}")
    assert (err <= allowed)[banded].all()
    tb, ab, _ = R.gelu_allowed(x, g, lowp=False)
    errb = ((g * (cdf + x * 0.3989422804014327 * e)).double() - tb).abs()
    assert (errb <= ab)[banded].all()


# ------------------------------------------------------------------------------------------------ the small kernels
def test_rows_add_reference():
    g_ = torch.Generator().manual_seed(1)
    a, b = R.ints(g_, (40, 8), -4, 4).double(), R.ints(g_, (25, 8), -4, 4).double()
    m = torch.randint(-1, 25, (40,), generator=g_, dtype=torch.int32)
    scale = torch.tensor([0.0, 1.0, 2.0, 1.0, 0.0, 2.0], dtype=torch.float64)
    ref = a.clone()
    for r in range(40):
        if m[r] >= 0:
            ref[r] += scale[r // 7] * b[m[r]]
    assert torch.equal(R.rows_add_ref(a, b, m, scale, 7), ref) and (m < 0).any()
    assert torch.equal(R.rows_add_ref(None, b), b)


@pytest.mark.parametrize("P", [4, 16])
def test_patchify_reference_equals_unfold(P):
    img, hw = R.patchify_operands(P, 4 + P)
    assert all(h % P or w % P or (h, w) == (64, 96) for h, w in hw.tolist()) and any(w % 4 for _, w in hw.tolist())
    for dt in (torch.float32, torch.float64):
        ref = R.patchify_ref(img, hw, P, dtype=dt)
        m = torch.tensor(R.PIXEL_MEAN, dtype=torch.float32).to(dt).view(1, 3, 1, 1)
        inv = (1 / torch.tensor(R.PIXEL_STD, dtype=torch.float32)).to(dt).view(1, 3, 1, 1)
        xn = (img.to(dt) - m) * inv
        for n, (h, w) in enumerate(hw.tolist()):
            xn[n, :, h:, :] = 0
            xn[n, :, :, w:] = 0
        un = F.unfold(xn, P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
        assert torch.equal(ref, un)
    # against the division by std in fp64: the fp32 reciprocal costs a relative 1e-7
    exact = (img.double() - torch.tensor(R.PIXEL_MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(R.PIXEL_STD, dtype=torch.float64).view(1, 3, 1, 1)
    assert (R.patchify_ref(img, hw, P, dtype=torch.float64)[: (64 // P) * (96 // P)].abs().max() - exact[0, :, :50, :70].abs().max()).abs() < 1e-5
    assert (R.patchify_ref(img, hw, P)[: (64 // P) * (96 // P)] == 0).any()


@pytest.mark.parametrize("L0,L1", R.LINEAR_CASES)
def test_linear_weights_equal_interpolate(L0, L1):
    g_ = torch.Generator().manual_seed(L0 + L1)
    t = torch.randn(L0, 6, generator=g_, dtype=torch.float64, requires_grad=True)
    ref = F.interpolate(t.t()[None], size=L1, mode="linear", align_corners=False)[0].t()
    W = R.linear_weights(L0, L1, coord=torch.float64)
    assert _close(W @ t.detach(), ref.detach())
    g = torch.randn(L1, 6, generator=g_, dtype=torch.float64)
    ref.backward(g)
    assert _close(W.t() @ g, t.grad)
    W32 = R.linear_weights(L0, L1)                       # the kernel's fp32 coordinate moves a weight by a few ulps of the coordinate
    assert (W32 - W).abs().max() <= 8 * 2.0 ** -24 * max(L0, 1) and _close(W32.sum(1), torch.ones(L1, dtype=torch.float64))
    assert torch.equal(R.linear_ref(t.detach(), L1), W32 @ t.detach()) and torch.equal(R.linear_ref(g, L1, backward_into=L0), W32.t() @ g)
    if L0 == L1:
        assert torch.equal(W32, torch.eye(L0, dtype=torch.float64))


@pytest.mark.parametrize("case", R.BICUBIC_CASES)
def test_cubic_weights_equal_interpolate(case):
    S0h, S0w, gh, gw = case
    g_ = torch.Generator().manual_seed(sum(case))
    t = torch.randn(S0h, S0w, 5, generator=g_, dtype=torch.float64, requires_grad=True)
    ref = F.interpolate(t.permute(2, 0, 1)[None], size=(gh, gw), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)
    Wy, Wx = R.cubic_weights(S0h, gh, coord=torch.float64), R.cubic_weights(S0w, gw, coord=torch.float64)
    assert _close(torch.einsum("ya,xb,abc->yxc", Wy, Wx, t.detach()), ref.detach())
    g = torch.randn(gh, gw, 5, generator=g_, dtype=torch.float64)
    ref.backward(g)
    assert _close(torch.einsum("ya,xb,yxc->abc", Wy, Wx, g), t.grad)
    assert (R.cubic_weights(S0h, gh) - Wy).abs().max() <= 64 * 2.0 ** -24 * S0h
    assert (R.bicubic_ref(t.detach(), gh, gw) - ref.detach()).abs().max() <= 1e-4 * ref.detach().abs().max()
    if (S0h, S0w) == (gh, gw):
        assert torch.equal(R.cubic_weights(S0h, gh), torch.eye(S0h, dtype=torch.float64)) and torch.equal(R.cubic_weights(S0h, gh, torch.float32), torch.eye(S0h))


def test_resize_cases_hold_the_edges():
    assert {(1, 1), (2, 7), (5, 1), (7, 14), (27, 9), (27, 27)} <= set(R.LINEAR_CASES)
    b = set(R.BICUBIC_CASES)
    assert any(c[:2] == (3, 5) and c[2:] != (3, 5) for c in b) and any(c[:2] == (5, 2) for c in b)                      # non-square sources
    assert any(c[:2] == (1, 1) for c in b) and any(c[:2] == (2, 2) for c in b) and any(c[2:] == (1, 1) for c in b)
    assert any(c[2] == 2 * c[0] and c[3] == 2 * c[1] for c in b) and any(c[0] == 3 * c[2] and c[1] == 3 * c[3] for c in b)


def test_maxpool_reference_equals_torch():
    x, g = R.maxpool_operands()
    y, tap = R.maxpool_ref(x)
    ty, ttap = R.maxpool_torch(x)
    assert R.same_bits(y, ty) and torch.equal(tap, ttap)
    # the operands hold what they promise: every non-empty subset of tied winners, both zeros, -inf everywhere, a NaN at every tap
    wins = x[0, :, :, 0].view(2, -1, 2).permute(1, 0, 2).reshape(-1, 4)
    ties = {tuple((w == 1).tolist()) for w in wins[:15]}
    assert len(ties) == 15 and all(any(t) for t in ties)
    zeros = {tuple(torch.signbit(w).tolist()) for w in wins[15:31]}
    assert len(zeros) == 16 and (wins[15:31] == 0).all() and (wins[31] == float("-inf")).all()
    nan_at = [int(torch.isnan(w).nonzero()[0]) for w in wins[32:]]
    assert sorted(set(nan_at)) == [0, 1, 2, 3] and all(torch.isnan(w).sum() == 1 for w in wins[32:])
    assert torch.isnan(y[0, 0, 32:, 0]).all() and tap[0, 0, 32:, 0].tolist() == nan_at
    assert set(tap[0, 0, :15].flatten().tolist()) == {0, 1, 2, 3}
    assert torch.signbit(y[0, 0, 15:31, 0]).tolist() == [bool(torch.signbit(w[0])) and bool(torch.signbit(w).all()) or bool(torch.signbit(w[0])) for w in wins[15:31]]
    # backward: autograd of max_pool2d on the NaN-free windows routes g to the same tap
    xr = x[:, :, : 2 * 32].permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 2, 2).backward(g[:, :, :32].permute(0, 3, 1, 2))
    dx = R.maxpool_bwd_ref(g, tap, 2, x.shape[2])
    assert torch.equal(dx[:, :, :64], xr.grad.permute(0, 2, 3, 1)) and (dx != 0).sum() == g.numel()
    assert R.same_bits(x, x.bfloat16().float()) and torch.equal(g, g.bfloat16().float())


@pytest.mark.parametrize("grad_scale", [1.0, 0.3])
def test_adamw_reference_equals_torch_on_a_double_parameter(grad_scale):
    h = R.adamw_hyper(grad_scale)
    for first, late in ((1, False), (1000, True), (100000, True)):
        p, g, m, v = (t.double() for t in R.adamw_operands(1000, first, late))
        pr = p.clone().requires_grad_(True)
        opt = torch.optim.AdamW([pr], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["wd"])
        opt.state[pr] = dict(step=torch.tensor(float(first - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        for step in range(first, first + (3 if first == 1 else 1)):
            pr.grad = g * h["grad_scale"]
            opt.step()
            r = R.adamw_ref(p, g, m, v, step, **h)
            assert _close(r["p"], pr.detach(), 1e-14) and _close(r["m"], opt.state[pr]["exp_avg"], 1e-14) and _close(r["v"], opt.state[pr]["exp_avg_sq"], 1e-14)
            p, m, v = r["p"], r["m"], r["v"]
    assert g[0] == 0 and R.adamw_operands(5, 1, False)[3][0] == 0 and h["lr"] != 1e-3 and h["lr"] == pytest.approx(1e-3, rel=1e-7)


# ------------------------------------------------------------------------------------------------ depthwise 7 x 7
@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("shape", R.DW_SHAPES)
def test_depthwise_references_equal_conv2d(shape, C):
    ops, ref = R.dw_case(shape, C)
    x = ops["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
    w = ops["wt"].double().permute(2, 0, 1).unsqueeze(1).requires_grad_(True)
    y = F.conv2d(x, w, ops["bias"].double(), padding=3, groups=C)
    y.backward(ops["g"].double().permute(0, 3, 1, 2))
    assert torch.equal(ref["y"], y.detach().permute(0, 2, 3, 1)) and torch.equal(ref["dgrad"], x.grad.permute(0, 2, 3, 1))
    assert torch.equal(ref["wgrad"], w.grad[:, 0].permute(1, 2, 0))
    assert torch.equal(ref["y_nobias"], ref["y"] - ops["bias"].double())
    for k in ("y", "dgrad", "wgrad"):                      # exact in fp32 too, and a single rounding to bf16 is defined
        R.round_to(ref[k], torch.bfloat16)
    y32 = F.conv2d(ops["x"].permute(0, 3, 1, 2), ops["wt"].permute(2, 0, 1).unsqueeze(1), ops["bias"], padding=3, groups=C)
    assert torch.equal(y32.double().permute(0, 2, 3, 1), ref["y"])


@pytest.mark.parametrize("C", R.DW_CHANNELS)
def test_depthwise_lattice_budget(C):
    for shape in R.DW_SHAPES:
        assert R.check_dw(R.dw_case(shape, C)[0]) < 2.0 ** -8


def test_depthwise_weight_gradient_launches():
    """(2, 13, 17) is the smallest multi-chunk map: 130 quads in 3 chunks of 44 on 8 chunk slots; a pixel lane's ping-pong loop ends on either buffer
    where the pixel lanes are fewer than the quads of a chunk"""
    p = R.dw_wgrad_plan(2, 13, 17, 264)
    assert (p["nquads"], p["chunks"], p["ppb"], p["slots"], p["npl"], p["dead_groups"]) == (130, 3, 44, 8, 8, 31) and p["ends"] == {0, 1}
    assert R.dw_wgrad_plan(2, 13, 17, 200)["ends"] == {0, 1} and R.dw_wgrad_plan(2, 13, 17, 200)["npl"] == 16
    assert R.dw_wgrad_plan(2, 13, 17, 8)["chunks"] == 3 and R.dw_wgrad_plan(2, 8, 13, 8)["chunks"] == 2 and R.dw_wgrad_plan(2, 5, 12, 8)["chunks"] == 1
    assert R.dw_groups(24) == (3, 2, 2) and R.dw_groups(200) == (25, 16, 2) and R.dw_groups(264) == (33, 32, 2) and R.dw_groups(8) == (1, 1, 1)
    interior = [(w0 >= 3 and w0 + 7 <= W) for _, _, W in R.DW_SHAPES for w0 in range(0, W, 4)]
    assert any(interior) and [any(w0 >= 3 and w0 + 7 <= 12 for w0 in range(0, 12, 4))] == [True]


# ------------------------------------------------------------------------------------------------ layer-scale add
def test_scale_add_reference_budget_and_row_tails():
    for C in R.DW_CHANNELS:
        ops, ref = R.sa_case(C, True)
        assert R.check_sa(ops) < 2.0 ** -8
        x, y, g = (ops[k].double().requires_grad_(k == "y") for k in ("x", "y", "g"))
        gamma = ops["gamma"].double().requires_grad_(True)
        s = ops["scale"].double()[torch.arange(R.SA_ROWS) // R.SA_ROWS_PER_SAMPLE][:, None]
        out = x + s * gamma * y
        out.backward(g)
        assert torch.equal(ref["out"], out.detach()) and torch.equal(ref["dy"], y.grad) and torch.equal(ref["dgamma"], gamma.grad)
        for k in ref:
            R.round_to(ref[k], torch.bfloat16 if k != "dgamma" else torch.float32)
    left = set()
    for knob in R.SA_KNOBS:
        p = R.sa_plan(R.SA_ROWS, 264, knob)
        left |= p["left"]
        assert p["last"] != p["rpb"] or knob == 1          # the row blocks get a tail
    assert left == {0, 1, 2, 3}
    assert R.sa_plan(R.SA_ROWS, 264, 512)["rpb"] == 56 and R.sa_plan(R.SA_ROWS, 264, 8)["rpb"] == 67 and R.sa_plan(R.SA_ROWS, 24, 1)["left"] >= {2, 3}

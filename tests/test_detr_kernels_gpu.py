"""The Deformable-DETR kernels (csrc/msda.hip, csrc/detr.hip) one by one against the references of detr_kernel_refs.py (pinned on the CPU
in test_detr_kernels_cpu.py).

  * multi-scale deformable attention, forward and backward, and every form of the self-attention value gradient (general scatter, gather
    walk with its far scatter, binned form, both overflow paths) on lattice operands: torch.equal with the explicit fp64 reference;
  * small attention, GroupNorm, the sampling glue, the box head's last step and the set criterion: per output tensor
    max|kernel - ref64| <= FACTOR * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|, ref32 / ref64 = the same torch function in fp32 / fp64 on the CPU.

The measured ratios are in the table below FACTOR.  Every check prints its figures before it asserts (pytest -s)."""
import numpy as np
import pytest
import torch

import detr_kernel_refs as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
# Measured on an MI355X: err_kernel / err_ref32, the largest over the cases of each test (`-`: both errors are zero).  No entry needed more than
# FACTOR, so the bound is FACTOR everywhere.
#
#   mha_small (5 shapes x 2 layouts, scores +-100, dropout)   out 1.19   lse 2.92   dq 1.81   dk 1.46   dv 1.47   delta 1.56
#   group_norm (7 shapes)                                     y 1.55     mean 2.45  rstd 4.51 dx 1.58   dgamma 5.22  dbeta 3.23
#   group_norm, x = randn + 10 (yardstick: torch fp32)        y 0.80     mean 1.02  rstd 0.86 dx 1.39   dgamma 0.21  dbeta 1.17
#   group_norm, x = randn + 30 (yardstick: torch fp32)        y 1.15     mean 1.28  rstd 0.77 dx 0.92   dgamma 0.09  dbeta 0.76
#   msda_prepare (3 shapes, logits +-80, with / without g_ref) loc 1.29  aw 1.97    g_raw 4.46  g_ref 2.30
#   box_finish (3 shapes, with / without g_ref)               boxes 1.06 g_t 1.00   g_ref 1.00
#   set criterion, logits in {0, +-30, +-100}                 losses 6.77  g_logits 1.00  g_boxes 1.00
#
# With the statistics as one fp32 pass of sum(x) and sum(x^2) and E[x^2] - m^2 (before they were centred on each chunk's mean) the same tests
# measured: x = randn + 10: y 20.4, rstd 139, dx 57.6; x = randn + 30: y 111, rstd 1124, dx 643; one value per group (1, 1, 32, 32):
# rstd 15.7 away from 316.2 (the variance was fl(x^2) - x^2 instead of 0).

@pytest.fixture(autouse=True)
def _tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _lib():
    from aldi_amd import _lib as L
    from aldi_amd.ops import _p, stream_ptr
    return L, _p, stream_ptr


class Check:
    """collects the fp64-matched comparisons of one test: prints every figure, fails at the end with all that missed"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def __call__(self, name, got, r32, r64, factor=FACTOR):
        got = got.detach().cpu().double().reshape(r64.shape)
        ek, er = (got - r64).abs().max().item(), (r32.double() - r64).abs().max().item()
        tol = R.tolerance(r32, r64, factor)
        finite = bool(torch.isfinite(got).all())
        print(f"RATIO {self.what:<44} {name:<9} err_kernel {ek:.3e} err_ref32 {er:.3e} ratio {ek / er if er else float('nan'):8.3f} tol {tol:.3e} max|ref| {r64.abs().max().item():.3e}")
        if not (finite and ek <= tol):
            self.bad.append((name, ek, er, tol))

    def done(self):
        assert not self.bad, (self.what, self.bad)


# ================================================================================================ 1. MSDA on lattice operands
def _levels(shapes):
    sh = torch.tensor(shapes, dtype=torch.int32)
    ls = torch.tensor(R.level_starts(shapes), dtype=torch.int32)
    return sh, ls


def _equal(got, ref, what):
    got = got.cpu().double().reshape(ref.shape)
    bad = got != ref
    assert not bad.any() and not torch.isnan(got).any(), (what, int(bad.sum()), int(torch.isnan(got).sum()), (got - ref).abs().nan_to_num(9e9).max().item())


@pytest.mark.parametrize("i", range(len(R.MSDA_CASES)))
def test_msda_forward_backward_equal_the_reference_on_lattice_operands(i):
    L, _p, stream_ptr = _lib()
    N, M, D, Lq, shapes, P = R.MSDA_CASES[i]
    ops, ref, _ = R.msda_case(i)
    S, Lv = ops["value"].shape[1], len(shapes)
    sh, ls = _levels(shapes)
    value, loc, attw, gout, sh, ls = (t.cuda() for t in (ops["value"], ops["loc"], ops["attw"], ops["gout"], sh, ls))
    nan = float("nan")
    out = torch.full((N, Lq, M * D), nan, device="cuda")
    L.call("aldi_ms_deform_attn_forward", _p(value), _p(sh), _p(ls), _p(loc), _p(attw), _p(out), N, S, M, D, Lq, Lv, P, stream_ptr())
    gv, gl, ga = torch.full_like(value, 7.0), torch.full_like(loc, nan), torch.full_like(attw, nan)
    L.call("aldi_ms_deform_attn_backward", _p(value), _p(sh), _p(ls), _p(loc), _p(attw), _p(gout), _p(gv), _p(gl), _p(ga), N, S, M, D, Lq, Lv, P, stream_ptr())
    assert L.last_dispatch() == "msda_bwd_value_scatter"
    torch.cuda.synchronize()
    _equal(out, ref[0], "out"); _equal(gv, ref[1], "grad_value"); _equal(gl, ref[2], "grad_loc"); _equal(ga, ref[3], "grad_attw")


def test_msda_refuses_head_dim_16():
    L, _p, stream_ptr = _lib()
    shapes = ((3, 3),)
    sh, ls = (t.cuda() for t in _levels(shapes))
    N, S, M, D, Lq, P = 1, 9, 1, 16, 4, 1
    value, loc, attw, gout = torch.zeros(N, S, M, D, device="cuda"), torch.zeros(N, Lq, M, 1, P, 2, device="cuda"), torch.zeros(N, Lq, M, 1, P, device="cuda"), torch.zeros(N, Lq, M * D, device="cuda")
    out, gv, gl, ga = torch.zeros_like(gout), torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attw)
    with pytest.raises(L.AldiHipError, match="head dim must be 32 or 64"):
        L.call("aldi_ms_deform_attn_forward", _p(value), _p(sh), _p(ls), _p(loc), _p(attw), _p(out), N, S, M, D, Lq, 1, P, stream_ptr())
    with pytest.raises(L.AldiHipError, match="head dim must be 32 or 64"):
        L.call("aldi_ms_deform_attn_backward", _p(value), _p(sh), _p(ls), _p(loc), _p(attw), _p(gout), _p(gv), _p(gl), _p(ga), N, S, M, D, Lq, 1, P, stream_ptr())


# ================================================================================================ 2. every value-gradient form
def _self_forms(Lv, pile):
    """(name, knobs, workspace, the dispatch expected)"""
    every = (1 << Lv) - 1
    forms = [("scatter", None, False, "msda_bwd_value_scatter"),
             ("walk-default", {}, False, "msda_bwd_value_gather"),
             ("walk-all", {"msda_gather": every}, False, "msda_bwd_value_gather"),
             ("walk-finest", {"msda_gather": 1}, False, "msda_bwd_value_gather"),
             ("walk-off", {"msda_gather": 0}, False, "msda_bwd_value_scatter")]
    forms += [(f"walk-list-{v}", {"msda_gather": every, "msda_gather_list": v}, False, "msda_bwd_value_gather") for v in R.GATHER_LISTS if v != 1500]
    forms += [("bin", {}, True, "msda_bwd_value_binned"), ("bin-small", {"msda_bin_list": 8}, True, "msda_bwd_value_binned")]
    if pile:
        forms = [f for f in forms if f[0] in ("scatter", "walk-default", "walk-all", "bin", "bin-small")]
    return forms


@pytest.mark.parametrize("name", ["nested", "ragged", "one", "eight", "pile", "d64"])
def test_self_attention_gradient_forms_equal_the_reference(name):
    """aldi_ms_deform_attn_backward_self in every form == the fp64 reference, bit for bit: grad_value of the general scatter, of the walk
    (default levels, all levels, the finest only, every tile size through msda_gather_list, an LDS list that overflows in `pile`), of the
    binned form (also with lists of capacity 256 that overflow), and grad_loc / grad_attw of each call"""
    L, _p, stream_ptr = _lib()
    pyr, N, M, D, P, _, one_point = R.SELF_CASES[name]
    shapes, ops, ref, _ = R.self_case(name)
    S, Lv = ops["value"].shape[1], len(shapes)
    sh, ls = _levels(shapes)
    host = np.ascontiguousarray(sh.numpy())
    value, loc, attw, gout, sh, ls = (t.cuda() for t in (ops["value"], ops["loc"], ops["attw"], ops["gout"], sh, ls))
    nan = float("nan")
    forms = _self_forms(Lv, one_point is not None)
    if D != 32:
        forms = [(n_, k_, w_, "msda_bwd_value_scatter") for n_, k_, w_, _ in forms if n_ in ("scatter", "walk-default", "bin")]
    for form, knobs, use_ws, dispatch in forms:
        L.reset_tuning()
        gv, gl, ga = torch.full_like(value, 7.0), torch.full_like(loc, nan), torch.full_like(attw, nan)
        if knobs is None:
            L.call("aldi_ms_deform_attn_backward", _p(value), _p(sh), _p(ls), _p(loc), _p(attw), _p(gout), _p(gv), _p(gl), _p(ga), N, S, M, D, S, Lv, P, stream_ptr())
        else:
            for k, v in knobs.items():
                L.set_tuning(k, v)
            ws = None
            if use_ws:
                need = int(L.lib.aldi_ms_deform_attn_backward_self_workspace(host.ctypes.data, N, S, M, Lv, P))
                assert need > 0
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            L.call("aldi_ms_deform_attn_backward_self", _p(value), _p(sh), _p(ls), host.ctypes.data, _p(loc), _p(attw), _p(gout), _p(gv), _p(gl), _p(ga),
                   _p(ws), 0 if ws is None else ws.numel(), N, S, M, D, Lv, P, stream_ptr())
        assert L.last_dispatch() == dispatch, (form, L.last_dispatch())
        torch.cuda.synchronize()
        _equal(gv, ref[1], (form, "grad_value")); _equal(gl, ref[2], (form, "grad_loc")); _equal(ga, ref[3], (form, "grad_attw"))


def test_self_attention_gradient_refuses_nine_levels():
    L, _p, stream_ptr = _lib()
    shapes = tuple(R.SELF_PYRAMIDS["eight"]) + ((1, 1),)
    N, M, D, P, S, Lv = 1, 1, 32, 1, sum(h * w for h, w in shapes), 9
    sh, ls = _levels(shapes)
    host = np.ascontiguousarray(sh.numpy())
    value, loc, attw, gout = torch.zeros(N, S, M, D, device="cuda"), torch.full((N, S, M, Lv, P, 2), 0.5, device="cuda"), torch.zeros(N, S, M, Lv, P, device="cuda"), torch.zeros(N, S, M * D, device="cuda")
    gv, gl, ga = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attw)
    assert int(L.lib.aldi_ms_deform_attn_backward_self_workspace(host.ctypes.data, N, S, M, Lv, P)) == 0
    with pytest.raises(L.AldiHipError, match="1 <= L <= 8"):
        L.call("aldi_ms_deform_attn_backward_self", _p(value), _p(sh.cuda()), _p(ls.cuda()), host.ctypes.data, _p(loc), _p(attw), _p(gout), _p(gv), _p(gl), _p(ga),
               None, 0, N, S, M, D, Lv, P, stream_ptr())


# ================================================================================================ 3. small attention
def _keep_mask(seed, shape, p):
    """the keep / (1 - p) factors the dropout kernels apply for (seed, element index)"""
    L, _p, stream_ptr = _lib()
    ones = torch.ones(shape, device="cuda")
    out = torch.empty_like(ones)
    L.call("aldi_dropout_add", _p(ones), None, _p(out), ones.numel(), p, seed, stream_ptr())
    return out


def _rows(t, ld, col0, width):
    """a NaN-filled [rows][ld] buffer holding t's rows at columns col0 .. col0 + width"""
    buf = torch.full((t.shape[0], ld), float("nan"), device="cuda")
    buf[:, col0:col0 + width] = t
    return buf


def _mha_kernels(q, k, v, do, B, Q, H, Dh, layout, drop_p=0.0, seed=0):
    """-> the six outputs on the CPU; packed: the model's layout, q | k in one [B Q][2 d] buffer (k = q + d, ld 2 d), v and dv [B Q][d];
    padded: every operand and gradient in its own buffer with rows of d + 12 floats.  Inputs' and outputs' unused columns are NaN before the
    calls and must be NaN after them."""
    L, _p, stream_ptr = _lib()
    d, T = H * Dh, B * Q
    scale = Dh ** -0.5
    q2, k2, v2, do2 = (t.reshape(T, d).cuda() for t in (q, k, v, do))
    nan = float("nan")
    if layout == "packed":
        qk = torch.cat([q2, k2], 1).contiguous()
        vb = v2.contiguous()
        dqk, dvb = torch.full((T, 2 * d), nan, device="cuda"), torch.full((T, d), nan, device="cuda")
        qp, kp, vp, dqp, dkp, dvp = qk.data_ptr(), qk.data_ptr() + 4 * d, vb.data_ptr(), dqk.data_ptr(), dqk.data_ptr() + 4 * d, dvb.data_ptr()
        ldq = ldk = lddq = lddk = 2 * d
        ldv = lddv = d
    else:
        ld = d + 12
        qb, kb, vb = _rows(q2, ld, 0, d), _rows(k2, ld, 0, d), _rows(v2, ld, 0, d)
        dqb, dkb, dvb = (torch.full((T, ld), nan, device="cuda") for _ in range(3))
        qp, kp, vp, dqp, dkp, dvp = (t.data_ptr() for t in (qb, kb, vb, dqb, dkb, dvb))
        ldq = ldk = ldv = lddq = lddk = lddv = ld
    out, lse, delta = torch.full((T, d), nan, device="cuda"), torch.full((B, H, Q), nan, device="cuda"), torch.full((B, H, Q), nan, device="cuda")
    L.call("aldi_mha_small_forward", qp, kp, vp, _p(out), _p(lse), B, Q, H, Dh, ldq, ldk, ldv, scale, drop_p, seed, stream_ptr())
    L.call("aldi_mha_small_backward", qp, kp, vp, _p(out), _p(do2), _p(lse), dqp, dkp, dvp, _p(delta), B, Q, H, Dh, ldq, ldk, ldv, lddq, lddk, lddv, scale, drop_p, seed,
           stream_ptr())
    torch.cuda.synchronize()
    if layout == "packed":
        dq, dk, dv = dqk[:, :d], dqk[:, d:], dvb
    else:
        dq, dk, dv = dqb[:, :d], dkb[:, :d], dvb[:, :d]
        for b in (dqb, dkb, dvb):
            assert torch.isnan(b[:, d:]).all()             # the columns outside the written ones keep the sentinel
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, delta=delta)


def _mha_check(what, B, Q, H, Dh, layout, spread=1.0, drop_p=0.0, seed=0):
    q, k, v, do = R.mha_operands(B, Q, H, Dh, 17 + Q, spread)
    keep = _keep_mask(seed, (B, H, Q, Q), drop_p).cpu() if drop_p else None
    if keep is not None:
        assert 0.85 < (keep != 0).float().mean().item() < 0.95 and set(keep.unique().tolist()) <= {0.0, keep.max().item()}
    r32, r64 = R.both(R.mha_ref, q, k, v, do, H=H, scale=Dh ** -0.5, keep=keep)
    got = _mha_kernels(q, k, v, do, B, Q, H, Dh, layout, drop_p, seed)
    c = Check(what)
    for name in ("out", "lse", "dq", "dk", "dv", "delta"):
        c(name, got[name], r32[name], r64[name])
    return c, r64, got


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("case", R.MHA_CASES)
def test_small_attention_forward_backward(case, layout):
    B, Q, H, Dh = case
    c, r64, got = _mha_check(f"mha {case} {layout}", B, Q, H, Dh, layout)
    if Q == 1:                                           # one key: p = 1, dq = dk = 0 (fp64 leaves a rounding of dP - delta), dv = dO
        assert r64["dq"].abs().max() < 1e-14 and r64["dk"].abs().max() < 1e-14
        assert got["dq"].abs().max().item() == 0 and got["dk"].abs().max().item() == 0
        assert torch.equal(got["dv"].cpu().double().view(-1), r64["dv"].view(-1))
    c.done()


def test_small_attention_scores_that_overflow_a_naive_exp():
    B, Q, H, Dh = 1, 65, 3, 32
    q, k, _, _ = R.mha_operands(B, Q, H, Dh, 17 + Q, 25.0)
    s = (q.view(B, Q, H, Dh).transpose(1, 2) @ k.view(B, Q, H, Dh).transpose(1, 2).transpose(-1, -2)) * Dh ** -0.5
    assert s.max().item() > 89 and s.min().item() < -89                             # exp(89) is past fp32
    c, _, _ = _mha_check("mha scores +-100", B, Q, H, Dh, "packed", spread=25.0)
    c.done()


def test_small_attention_with_dropout():
    c, _, _ = _mha_check("mha dropout 0.1", 2, 127, 2, 32, "packed", drop_p=0.1, seed=12345)
    c.done()


# ================================================================================================ 3. / 4. GroupNorm
def _gn_kernels(x, gamma, beta, gy, dgamma0, dbeta0, G, eps=R.GN_EPS):
    L, _p, stream_ptr = _lib()
    N, HW, C = x.shape
    x, gamma, beta, gy = (t.cuda() for t in (x, gamma, beta, gy))
    dgamma, dbeta = dgamma0.cuda().clone(), dbeta0.cuda().clone()
    nan = float("nan")
    y, dx = torch.full_like(x, nan), torch.full_like(x, nan)
    mean, rstd = torch.full((N, G), nan, device="cuda"), torch.full((N, G), nan, device="cuda")
    ws = torch.empty(max(int(L.lib.aldi_group_norm_workspace(N, HW, G)), 4), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(int(L.lib.aldi_group_norm_backward_workspace(N, HW, C, G)), dtype=torch.uint8, device="cuda")
    L.call("aldi_group_norm_forward", _p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), _p(ws), N, HW, C, G, eps, stream_ptr())
    L.call("aldi_group_norm_backward", _p(gy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta), _p(ws2), N, HW, C, G, stream_ptr())
    torch.cuda.synchronize()
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


GN_OUTPUTS = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


@pytest.mark.parametrize("case", R.GN_CASES)
def test_group_norm_forward_backward(case):
    N, HW, C, G = case
    ops = R.gn_operands(N, HW, C, G, 40 + HW % 97)
    r32, r64 = R.both(R.gn_ref, *ops, G=G)
    got = _gn_kernels(*ops, G)
    c = Check(f"group_norm {case}")
    for name in GN_OUTPUTS:
        c(name, got[name], r32[name], r64[name])
    if HW * (C // G) == 1:                               # one value per group: y = beta, rstd = eps^-1/2
        assert torch.equal(got["y"].cpu(), ops[2].expand(N, HW, C))
        assert (got["rstd"].cpu().double() * float(torch.tensor(R.GN_EPS).double().sqrt()) - 1).abs().max().item() <= 2.0 ** -22
    if case == R.GN_CASES[0]:                            # deterministic: a second run gives the same bits
        again = _gn_kernels(*ops, G)
        for name in GN_OUTPUTS:
            assert torch.equal(got[name], again[name]), name
    c.done()


@pytest.mark.parametrize("c_off", [10.0, 30.0])
def test_group_norm_on_offset_inputs(c_off):
    """x = randn + c at the input projections' shape; the yardstick is torch's own fp32 group_norm and its autograd.
    What this test measured before the statistics were centred on each chunk's mean is in the table at the top of the file."""
    N, HW, C, G = 2, 1961, 256, 32
    ops = R.gn_operands(N, HW, C, G, 50 + int(c_off), offset=c_off, std=1.0)
    r64 = R.gn_ref(*(t.double() for t in ops), G)
    t32 = R.gn_torch(*ops, G)
    got = _gn_kernels(*ops, G)
    c = Check(f"group_norm offset {c_off:g}")
    for name in GN_OUTPUTS:
        c(name, got[name], t32[name], r64[name])
    c.done()


def test_group_norm_argument_errors():
    L, _p, stream_ptr = _lib()
    x = torch.zeros(1, 4, 8192, device="cuda")
    v, st = torch.zeros(8192, device="cuda"), torch.zeros(64, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for C, G in ((24, 5), (6, 3), (4100, 4)):            # C % G != 0, C % 4 != 0, C > 4096
        with pytest.raises(L.AldiHipError, match="group_norm_forward: bad args"):
            L.call("aldi_group_norm_forward", _p(x), _p(v), _p(v), _p(x), _p(st), _p(st), _p(ws), 1, 4, C, G, 1e-5, stream_ptr())
        with pytest.raises(L.AldiHipError, match="group_norm_backward: bad args"):
            L.call("aldi_group_norm_backward", _p(x), _p(x), _p(v), _p(st), _p(st), _p(x), _p(v), _p(v), _p(ws), 1, 4, C, G, stream_ptr())


# ================================================================================================ 3. the sampling glue
@pytest.mark.parametrize("with_ref", [True, False])
@pytest.mark.parametrize("case,span", [(R.PREPARE_CASES[0], 1.0), (R.PREPARE_CASES[1], 1.0), (R.PREPARE_CASES[2], 1.0), (R.PREPARE_CASES[2], 25.0)])
def test_sampling_glue_forward_backward(case, span, with_ref):
    L, _p, stream_ptr = _lib()
    T, M, Lv, P = case
    raw, ref, g_loc, g_aw = R.prepare_operands(T, M, Lv, P, 60 + T, span)
    LP = Lv * P
    if span > 1:                                         # logits spanning +-80
        raw[0, M * LP * 2], raw[0, M * LP * 2 + 1] = 80.0, -80.0
        assert raw[:, M * LP * 2:].max().item() >= 80 and raw[:, M * LP * 2:].min().item() <= -80
    shapes = R.PREPARE_SHAPES
    r32, r64 = R.both(R.prepare_ref, raw, ref, g_loc, g_aw, shapes=shapes, M=M, L=Lv, P=P)
    sh = torch.tensor(shapes[:Lv], dtype=torch.int32).cuda()
    nan = float("nan")
    raw_d, ref_d, gl_d, ga_d = (t.cuda() for t in (raw, ref, g_loc, g_aw))
    loc, aw = torch.full((T, M, Lv, P, 2), nan, device="cuda"), torch.full((T, M, Lv, P), nan, device="cuda")
    L.call("aldi_msda_prepare", _p(raw_d), _p(ref_d), _p(sh), _p(loc), _p(aw), T, M, Lv, P, stream_ptr())
    g_raw = torch.full_like(raw_d, nan)
    g_ref = torch.full((T, Lv, 2), nan, device="cuda") if with_ref else None
    L.call("aldi_msda_prepare_backward", _p(gl_d), _p(ga_d), _p(aw), _p(sh), _p(g_raw), _p(g_ref), T, M, Lv, P, stream_ptr())
    torch.cuda.synchronize()
    c = Check(f"msda_prepare {case} span {span:g} g_ref {with_ref}")
    c("loc", loc, r32["loc"], r64["loc"]); c("aw", aw, r32["aw"], r64["aw"]); c("g_raw", g_raw, r32["g_raw"], r64["g_raw"])
    if with_ref:
        c("g_ref", g_ref, r32["g_ref"], r64["g_ref"])
    if LP == 1:                                          # one sample: the weight is 1 and the logit gradient 0
        assert torch.equal(aw.cpu(), torch.ones(T, M, Lv, P)) and g_raw[:, M * LP * 2:].abs().max().item() == 0
    c.done()


# ================================================================================================ 3. the box head's last step
@pytest.mark.parametrize("with_ref", [True, False])
@pytest.mark.parametrize("rows,refs", [(300, 100), (1, 1), (257, 257)])
def test_box_finish_forward_backward(rows, refs, with_ref):
    L, _p, stream_ptr = _lib()
    t, ref, g_boxes, g_ref0 = R.box_operands(rows, refs, 70 + rows)
    r32, r64 = R.both(R.box_ref, t, ref, g_boxes, g_ref0)
    nan = float("nan")
    t_d, ref_d, gb_d = (x.cuda() for x in (t, ref, g_boxes))
    boxes, g_t = torch.full((rows, 4), nan, device="cuda"), torch.full((rows, 4), nan, device="cuda")
    g_ref = g_ref0.cuda().clone() if with_ref else None
    L.call("aldi_detr_box_finish", _p(t_d), _p(ref_d), _p(boxes), rows, refs, stream_ptr())
    L.call("aldi_detr_box_finish_backward", _p(gb_d), _p(boxes), _p(ref_d), _p(g_t), _p(g_ref), rows, refs, stream_ptr())
    torch.cuda.synchronize()
    c = Check(f"box_finish R {rows} refs {refs} g_ref {with_ref}")
    c("boxes", boxes, r32["boxes"], r64["boxes"]); c("g_t", g_t, r32["g_t"], r64["g_t"])
    if with_ref:
        c("g_ref", g_ref, r32["g_ref"], r64["g_ref"])
    c.done()


# ================================================================================================ 3. mask_rows
@pytest.mark.parametrize("T,C", [(1, 4), (333, 256), (5000, 1024)])
def test_mask_rows(T, C):
    L, _p, stream_ptr = _lib()
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, C, generator=g)
    keep = (torch.rand(T, generator=g) < 0.6).to(torch.uint8)
    if T == 1:
        keep[0] = 0
    else:
        keep[0], keep[1], keep[T - 1] = 0, 1, 0
    x[0, 0], x[0, C - 1], x[T - 1, C // 2] = float("nan"), float("inf"), float("-inf")
    if T > 1:
        x[1, 1], x[1, 2] = float("nan"), float("inf")    # a kept row keeps them
    x_d = x.cuda()
    L.call("aldi_mask_rows", _p(x_d), _p(keep.cuda()), T, C, stream_ptr())
    got = x_d.cpu()
    kept = keep.bool()
    assert torch.equal(got[kept].view(torch.int32), x[kept].view(torch.int32))
    assert (got[~kept].view(torch.int32) == 0).all()


# ================================================================================================ 3. the set criterion at saturated logits
def test_set_criterion_at_saturated_logits():
    from aldi_amd.detr.criterion import SetCriterion
    from oracle import deformable_detr as D
    logits, boxes, targets = R.criterion_operands(11)
    Ld, B, Nq, K = logits.shape
    tg64 = [{"labels": t["labels"], "boxes": t["boxes"].double()} for t in targets]
    indices = [D.hungarian_match(logits[l].double(), boxes[l].double(), tg64) for l in range(Ld)]
    match = torch.full((Ld, B, Nq), -1, dtype=torch.int32)
    for l in range(Ld):
        for b, (qi, gi) in enumerate(indices[l]):
            match[l, b, qi] = gi.to(torch.int32)
    assert (match >= 0).sum().item() == Ld * sum(len(t["labels"]) for t in targets) and (match < 0).any()
    r32, r64 = (R.criterion_ref(logits.to(dt), boxes.to(dt), targets, indices) for dt in (torch.float32, torch.float64))
    out, gl, gb = SetCriterion()(logits.cuda(), boxes.cuda(), targets, match=match.view(Ld * B, Nq).cuda())
    torch.cuda.synchronize()
    got = torch.stack([torch.stack([out[k + ("" if l == Ld - 1 else f"_{l}")] for k in ("loss_ce", "loss_bbox", "loss_giou")]) for l in range(Ld)])
    assert torch.isfinite(got).all() and torch.isfinite(gl).all() and torch.isfinite(gb).all()
    c = Check("set criterion, logits in {0, +-30, +-100}")
    c("losses", got, r32["losses"], r64["losses"]); c("g_logits", gl, r32["g_logits"], r64["g_logits"]); c("g_boxes", gb, r32["g_boxes"], r64["g_boxes"])
    c.done()

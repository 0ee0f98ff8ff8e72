"""The RoIAlign kernels (csrc/roi.hip) one by one against the fp64 reference of roialign_exact.py (pinned on the CPU in
test_roialign_exact_cpu.py).

  * lattice cases (samples exactly at -1, 0, H - 1, H and on integers, ROIs over every corner and outside the map, degenerate boxes, bins
    from a quarter pixel to 64 pixels, P in {1, 2, 5, 7}, ragged maps, the 208 x 344 limit of the separable forward, the level thresholds,
    a 257-ROI image for the gathers' scan and pipeline): torch.equal with the reference for the separable and the vector forward on fp32
    and bf16 maps, the scatter backward, the one-row gather on fp32 and bf16 pooled gradients and the two-row gather, the gathers into
    NaN-prefilled fp32 and bf16 gradient maps;
  * random boxes: max|kernel - ref64| <= FACTOR * max|oracle32 - ref64| (+ half a bf16 ulp of the reference value for a bf16 output),
    oracle32 = the oracle's fp32 roi_pool and its autograd gradient on the same operands;
  * rois_from_proposals: padding rows carry index -1 and pool to exact zeros.

Measured on an MI355X, err_kernel / err_oracle32 on the random boxes (FACTOR = 8; every check prints its figures before it asserts, pytest -s):

  forward, separable       fp32 maps 0.99   bf16 maps 0.65
  forward, vector          fp32 maps 1.00   bf16 maps 0.65
  scatter backward         fp32 pooled 1.00 bf16 pooled 1.00                      (worst of the four levels)
  one-row gather           fp32 pooled 1.00 bf16 pooled 1.00   bf16 pooled into bf16 maps 0.44
  two-row gather           bf16 pooled into fp32 maps 1.00     into bf16 maps 0.44

err_oracle32 is 1.4e-5 forward and 1.2e-5 / 5.1e-6 / 1.8e-6 / 2.6e-6 on the four gradient maps (max|ref| about 2.5): the fp32 rounding of the level
coordinates, which the oracle and every kernel share, so the ratios sit at 1; no entry needed more than FACTOR.  The 26 tests take 5.5 s on an
MI355X, the slowest (the random boxes) 1.7 s.  Every lattice case was bit-exact on the first run.
"""
import pytest
import torch

import roialign_exact as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _equal(got, ref, what):
    got = got.float().cpu().double()
    bad = got != ref
    assert not bad.any() and not torch.isnan(got).any(), (what, int(bad.sum()), int(torch.isnan(got).sum()), (got - ref).abs().nan_to_num(9e9).max().item(),
                                                           bad.nonzero()[:4].tolist())


def _forward(feats, rois, P, dtype, sep):
    from aldi_amd import ops, _lib as L
    try:
        L.reset_tuning(); L.set_tuning("roialign_sep", sep)
        fd = [f.to(DEV, dtype) for f in feats]
        pooled = torch.full((len(rois), P, P, R.C), NAN, dtype=dtype, device=DEV)
        ops.roialign(ops.make_roi_feats(fd, None, R.SCALES), rois.to(DEV), len(rois), P, pooled, backward=False)
        torch.cuda.synchronize()
    finally:
        L.reset_tuning()
    return pooled


def _backward(shapes, N, rois, P, gp, kernel, gdt, rois_sorted=False):
    """kernel: 'scatter' (zero-initialised fp32 maps), 'gather1' / 'gather2' (NaN-prefilled maps of type gdt)"""
    from aldi_amd import ops, _lib as L
    try:
        L.reset_tuning()
        fd = [torch.zeros(N, h, w, R.C, dtype=gp.dtype, device=DEV) for h, w in shapes]
        rd, gd = rois.to(DEV), gp.to(DEV)
        if kernel == "scatter":
            maps = [torch.zeros(N, h, w, R.C, dtype=torch.float32, device=DEV) for h, w in shapes]
            ops.roialign(ops.make_roi_feats(fd, maps, R.SCALES), rd, len(rois), P, gd, backward=True)
        else:
            L.set_tuning("roialign_bwd_rows", 1 if kernel == "gather1" else 2)
            maps = [torch.full((N, h, w, R.C), NAN, dtype=gdt, device=DEV) for h, w in shapes]
            ops.roialign_backward(ops.make_roi_feats(fd, maps, R.SCALES), rd, len(rois), P, gd, N, rois_sorted=rois_sorted, grad_dtype=gdt)
        torch.cuda.synchronize()
    finally:
        L.reset_tuning()
    return maps


# (kernel, pooled-gradient type, gradient-map type)
BACKWARDS = (("scatter", torch.float32, torch.float32), ("scatter", torch.bfloat16, torch.float32), ("gather1", torch.float32, torch.float32), ("gather1", torch.bfloat16, torch.float32),
             ("gather1", torch.bfloat16, torch.bfloat16), ("gather2", torch.bfloat16, torch.float32), ("gather2", torch.bfloat16, torch.bfloat16))


# ================================================================================================ lattice cases
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_forward_equals_the_reference_on_lattice_operands(name):
    c = R.cases()[name]
    feats, _ = R.operands(name)
    ref = R.reference(name)[0]
    rois = c.forward_rois()
    for sep in (1, 0):                                  # the separable form (maps above 208 x 344 take the vector form by themselves), the vector form
        for dtype in (torch.float32, torch.bfloat16):
            got = _forward(feats, rois, c.P, dtype, sep)
            _equal(got, ref if dtype == torch.float32 else ref.to(torch.bfloat16).double(), (name, sep, dtype))


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_backward_equals_the_reference_on_lattice_operands(name):
    c = R.cases()[name]
    _, gp = R.operands(name)
    ref = R.reference(name)[1]
    orders = [(c.rois, gp, c.rois_sorted)]
    if c.rois_sorted:                                   # the same rows shuffled: every workgroup scans all of them
        perm = torch.randperm(c.R, generator=torch.Generator().manual_seed(5))
        orders.append((c.rois[perm].contiguous(), gp[perm].contiguous(), False))
    for rois, g, srt in orders:
        for kernel, pdt, gdt in BACKWARDS:
            maps = _backward(c.shapes, c.N, rois, c.P, g.to(pdt), kernel, gdt, srt)
            for l in range(4):
                _equal(maps[l], ref[l] if gdt == torch.float32 else ref[l].to(torch.bfloat16).double(), (name, kernel, pdt, gdt, srt, l))


# ================================================================================================ random boxes
def test_every_kernel_is_within_8x_of_the_oracles_fp32_error_on_random_boxes():
    b = R.bounded_case()
    bad = []

    def check(what, got, r32, r64, lowp):
        ok, ek, e32 = R.bound(got.float(), r32, r64, lowp)
        print(f"RATIO {what:<46} err_kernel {ek:.3e} err_oracle32 {e32:.3e} ratio {ek / e32:7.3f} max|ref| {r64.abs().max().item():.3e}")
        if not ok:
            bad.append((what, ek, e32))
    for sep in (1, 0):
        for dtype in (torch.float32, torch.bfloat16):
            got = _forward(b["feats"], b["rois"], b["P"], dtype, sep)
            check(f"forward {'separable' if sep else 'vector'} {dtype}", got, b["out32"], b["out64"], dtype == torch.bfloat16)
    for kernel, pdt, gdt in BACKWARDS:
        maps = _backward(R.BOUNDED_SHAPES, b["N"], b["rois"], b["P"], b["gp"].to(pdt), kernel, gdt, True)
        for l in range(4):
            check(f"{kernel} pooled {pdt} maps {gdt} level {l}", maps[l], b["G32"][l], b["G64"][l], gdt == torch.bfloat16)
    assert not bad, bad


# ================================================================================================ rois_from_proposals
def test_rois_from_proposals_padding_rows_pool_to_exact_zeros():
    from aldi_amd import ops
    P, N = 7, 3
    c = R.cases()["edges"]
    feats = [f[:1].expand(N, -1, -1, -1).contiguous() for f in R.operands("edges")[0]]
    props = torch.zeros(N, P, 4)
    props[1, 0] = c.rois[14, 1:]
    props[2] = c.rois[[0, 2, 4, 7, 14, 16, 20], 1:]
    props[0] = c.rois[:P, 1:]                           # image 0 counts no proposal: its boxes must not be read as ROIs
    props[1, 1:] = c.rois[1:P, 1:]
    pcount = torch.tensor([0, 1, P], dtype=torch.int32)
    rois = torch.full((N * P, 5), NAN, device=DEV)
    ops.rois_from_proposals(props.to(DEV), pcount.to(DEV), P, N, rois)
    torch.cuda.synchronize()
    want = torch.zeros(N * P, 5)
    want[:, 0] = -1
    want[P] = torch.cat([torch.tensor([1.0]), props[1, 0]])
    want[2 * P:] = torch.cat([torch.full((P, 1), 2.0), props[2]], 1)
    assert torch.equal(rois.cpu(), want)
    ref = R.ref_forward(feats, want, 7)
    assert ref[P].any() and ref[2 * P:].any() and not ref[:P].any() and not ref[P + 1:2 * P].any()
    for sep in (1, 0):
        for dtype in (torch.float32, torch.bfloat16):
            got = _forward(feats, rois.cpu(), 7, dtype, sep)
            _equal(got, ref if dtype == torch.float32 else ref.to(torch.bfloat16).double(), (sep, dtype))
            assert not got[:P].float().abs().sum().item() and not got[P + 1:2 * P].float().abs().sum().item()

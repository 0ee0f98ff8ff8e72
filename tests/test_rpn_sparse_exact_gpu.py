"""The sparse RPN-head backward on the device against rpn_sparse_refs.py, bit for bit: the three entry points called directly through ops
on a tiny five-level pyramid (aldi_rpn_active_pixels: the ascending list, its count, the cap overflow; aldi_rpn_sparse_gather: converted
and bit-copied rows, zero taps outside the level, zero rows past the count; aldi_rpn_sparse_scatter: every thread grouping, every owner
case, fp32 and bf16 maps, the single rounding of bf16 maps, repeatability).  No tolerance anywhere."""
import pytest
import torch

import rpn_sparse_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7
F32, BF16 = torch.float32, torch.bfloat16


def _geom():
    from aldi_amd import ops
    return ops.make_geom(R.LEVELS, 1, R.CH)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------
# active list
# ------------------------------------------------------------------------------------------------
def _active(ghead, cap):
    from aldi_amd import ops
    geom = _geom()
    gd = ghead.to(DEV)
    idx, count, err = torch.full((cap,), SENT, dtype=torch.int32, device=DEV), _i32([SENT]), _i32([0])
    ws = torch.full((ops.rpn_active_pixels_workspace(geom, R.N),), 0x5A, dtype=torch.uint8, device=DEV)
    ops.rpn_active_pixels(geom, R.level_views(gd), R.N, cap, idx, count, ws, err)
    torch.cuda.synchronize()
    return idx.cpu(), int(count.cpu()), int(err.cpu())


@pytest.mark.parametrize("kind", R.ACTIVE_PATTERNS)
def test_active_list_is_the_ascending_nonzero_rows(kind):
    ghead = R.ghead_pattern(kind)
    ref = R.active_ref(ghead)
    cap = R.TOTAL + 3
    idx, count, err = _active(ghead, cap)
    assert count == ref.numel() and err == 0
    assert torch.equal(idx[:count].long(), ref) and bool((idx[count:] == SENT).all())


@pytest.mark.parametrize("kind,cap", [("all", 100), ("all", 4096), ("all", R.TOTAL - 1), ("all", R.TOTAL), ("boundaries", 10), ("boundaries", 9),
                                      ("boundaries", 3), ("boundaries", 1), ("first", 1)])
def test_active_list_cap(kind, cap):
    """more active pixels than the caller's bound: the first `cap` rows, the TRUE count, and the overflow flag (value 2) and nothing else in
    err; a list that just fits leaves err alone"""
    ghead = R.ghead_pattern(kind)
    ref = R.active_ref(ghead)
    idx, count, err = _active(ghead, cap)
    kept = min(cap, ref.numel())
    assert count == ref.numel()
    assert torch.equal(idx[:kept].long(), ref[:kept]) and bool((idx[kept:] == SENT).all())
    assert err == (2 if ref.numel() > cap else 0)


# ------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Cf", [(BF16, 8), (BF16, 24), (BF16, 256), (F32, 4), (F32, 8), (F32, 256)])
def test_gather_rows_are_converted_and_copied_bit_for_bit(T, Cf):
    from aldi_amd import ops
    rows = R.pixel_rows()
    cap = len(rows) + 5
    ghead = torch.randn(R.TOTAL, R.CH, generator=torch.Generator().manual_seed(Cf))
    hidden, feat = R.random_bits((R.TOTAL, Cf), T, Cf + 1), R.random_bits((R.TOTAL, Cf), T, Cf + 2)
    ref = R.gather_ref(rows, cap, ghead, hidden, feat)
    gd, hd, fd = ghead.to(DEV), hidden.to(DEV), feat.to(DEV)
    assert torch.equal(R.as_int(fd.cpu()), R.as_int(feat))                        # (the upload keeps NaN payloads)
    idx = torch.full((cap,), 0, dtype=torch.int32, device=DEV)
    idx[:len(rows)] = _i32(rows)
    out = [torch.empty(s, dtype=torch.uint8, device=DEV).fill_(0xFF) for s in
           (cap * R.CH * T.itemsize, cap * Cf * T.itemsize, cap * 9 * Cf * T.itemsize)]
    G, Tm, X9 = (o.view(T) for o in out)
    ops.rpn_sparse_gather(_geom(), R.level_views(gd), R.level_views(hd), R.level_views(fd), R.N, Cf, cap, idx, _i32([len(rows)]), G, Tm, X9)
    torch.cuda.synchronize()
    for name, got, want in zip(("G", "Tm", "X9"), (G, Tm, X9), ref):
        assert torch.equal(R.as_int(got.cpu().view(want.shape)), R.as_int(want)), name


# ------------------------------------------------------------------------------------------------
# scatter
# ------------------------------------------------------------------------------------------------
def _scatter(rows, cap, Y, prefill, times=1):
    from aldi_amd import ops
    geom, Cf = _geom(), Y.shape[2]
    idx = torch.full((cap,), 0, dtype=torch.int32, device=DEV)
    idx[:len(rows)] = _i32(rows)
    count, Yd, outs = _i32([len(rows)]), Y.to(DEV), []
    for _ in range(times):
        m = prefill.to(DEV)
        ops.rpn_sparse_scatter(geom, R.level_views(m), Yd, R.N, Cf, cap, idx, count)
        torch.cuda.synchronize()
        outs.append(m.cpu())
    return outs


@pytest.mark.parametrize("Ty,Tm", [(F32, F32), (BF16, F32), (BF16, BF16)])
@pytest.mark.parametrize("Cf", [8, 24, 256, 2040, 2048])
def test_scatter_equals_the_definition(Cf, Ty, Tm):
    """integer rows into integer maps: the fp64 definition is exact, fp32 maps and (results <= 256) bf16 maps are bit-equal; targets nobody
    reaches keep their bits; a second run from the same inputs gives the same bits.  Cf = 8, 24, 256, 2040, 2048: 1, 3, 32, 255, 256 threads
    and 256, 85, 8, 1, 1 groups per workgroup (at 8 groups the ninth tap is a second round)"""
    rows = R.pixel_rows()
    cap = len(rows) + 4
    Y, pre = R.y_exact(cap, len(rows), Cf, Ty), R.prefill_exact(Cf, Tm)
    ref = R.scatter_ref(rows, Y, pre)
    first, second = _scatter(rows, cap, Y, pre, times=2)
    assert torch.equal(R.as_int(first), R.as_int(ref))
    assert torch.equal(R.as_int(second), R.as_int(first))
    reached = R.scatter_delta(rows, Y)[1]
    assert torch.equal(R.as_int(first)[~reached], R.as_int(pre)[~reached]) and not torch.equal(R.as_int(first)[reached], R.as_int(pre)[reached])


@pytest.mark.parametrize("Cf", [8, 24, 256, 2048])
def test_scatter_rounds_bf16_maps_once(Cf):
    """results between bf16 values, both kinds of tie included (257 -> 256, 259 -> 260): the exact sum rounded once to nearest-even, i.e.
    the contributions are summed in fp32 and the map is rounded when it is written -- a map rounded per contribution sticks at 256"""
    rows = R.pixel_rows()
    cap = len(rows) + 4
    Y, pre = R.y_ones(cap, len(rows), Cf), R.prefill_ties(Cf)
    ref = R.scatter_ref(rows, Y, pre)
    (got,) = _scatter(rows, cap, Y, pre)
    t = R.row_of(2, 0, 1, 1)
    assert ref[t, :4].float().tolist() == [256.0, 258.0, 260.0, 260.0]
    assert got[t, :4].float().tolist() == ref[t, :4].float().tolist()
    assert torch.equal(R.as_int(got), R.as_int(ref))

"""Pins rpn_sparse_refs.py without a GPU: the geometry puts the boundaries where the kernels' segment and ballot logic can go wrong, the
scatter reference IS the data gradient of the dense 3x3 convolution (torch.autograd, fp64: this fixes the tap orientation independently of
the kernel), every operand meets the precondition of bit equality, and wrong variants of the references differ exactly at the edge."""
import pytest
import torch

import rpn_sparse_refs as R


def test_geometry_puts_boundaries_inside_segments_and_ballot_words():
    assert R.ROW0 == [0, 4160, 5200, 5224, 5232, 5234] and R.TOTAL == 5234
    assert R.ROW0[1] > R.SEG and -(-R.TOTAL // R.SEG) == 2                    # more than one segment; level 0 crosses the segment boundary
    assert [b % 64 for b in R.ROW0[2:-1]] == [16, 40, 48] and all(b % R.SEG for b in R.ROW0[1:-1])
    assert R.BOUNDARY_ROWS == [4095, 4096, 4159, 4160, 5199, 5200, 5223, 5224, 5231, 5232]
    for row in (0, 4159, 4160, 5199, 5200, 5233):
        assert R.row_of(*R.pixel_of(row)) == row
    assert R.pixel_of(4159) == (0, 1, 39, 51) and R.pixel_of(4160) == (1, 0, 0, 0) and R.pixel_of(5233) == (4, 1, 0, 0)
    v = R.level_views(torch.arange(R.TOTAL * 2).view(R.TOTAL, 2))
    assert [tuple(t.shape) for t in v] == [(2, h, w, 2) for h, w in R.LEVELS] and int(v[2][1, 2, 3, 0]) == 2 * R.row_of(2, 1, 2, 3)


def test_active_patterns():
    want = {"none": [], "first": [0], "last": [R.TOTAL - 1], "last_channel": [3, 64, 4095, 4160, 5201], "neg_zero": [], "nan": [4101],
            "denormal": [70, 5233], "boundaries": R.BOUNDARY_ROWS}
    assert set(want) | {"all"} == set(R.ACTIVE_PATTERNS)
    for kind, rows in want.items():
        assert R.active_ref(R.ghead_pattern(kind)).tolist() == rows, kind
    assert R.active_ref(R.ghead_pattern("all")).tolist() == list(range(R.TOTAL))
    nz = R.ghead_pattern("neg_zero")
    assert int((nz.view(torch.int32) != 0).sum()) == 4 * R.CH + 1                # the -0.0 are there, as bits
    d = R.ghead_pattern("denormal")
    assert 0 < float(d[70, 2]) < 1.2e-38 and float(d[5233, 15]) < 0          # sub-normal fp32, not flushed by the reference


def test_pixels_cover_the_corners_edges_and_small_levels():
    rows = R.pixel_rows()
    px = [R.pixel_of(r) for r in rows]
    assert rows == sorted(rows) and len(rows) == 28 + 3 + 24 + 8 + 1
    for l, (H, W) in enumerate(R.LEVELS[:1]):
        for h, w in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert (l, 0, h, w) in px
        assert any(p[2] == 0 and 0 < p[3] < W - 1 for p in px) and any(p[2] == H - 1 and 0 < p[3] < W - 1 for p in px)
        assert any(p[3] == 0 and 0 < p[2] < H - 1 for p in px) and any(p[3] == W - 1 and 0 < p[2] < H - 1 for p in px)
    assert sum(p[0] == 2 for p in px) == 24 and sum(p[0] == 3 for p in px) == 8 and (4, 1, 0, 0) in px and (4, 0, 0, 0) not in px
    assert R.row_of(0, 0, 39, 51) + 1 == R.row_of(0, 1, 0, 0) and {R.row_of(0, 0, 39, 51), R.row_of(0, 1, 0, 0)} <= set(rows)
    # targets reached by 1 .. 9 contributions all occur
    ones = torch.ones(len(rows), 9, 1)
    delta, reached = R.scatter_delta(rows, ones)
    assert sorted(set(delta[reached, 0].tolist())) == [1.0, 2.0, 3.0, 4.0, 6.0, 9.0]
    assert int(reached.sum()) < R.TOTAL // 10 and bool((delta[~reached] == 0).all())


def test_scatter_reference_is_the_data_gradient_of_the_dense_convolution():
    rows = R.pixel_rows()
    g = torch.Generator().manual_seed(0)
    Co, Ci = 3, 4
    g_t = torch.randint(-3, 4, (len(rows), Co), generator=g)
    Wt = torch.randint(-4, 5, (Co, Ci, 3, 3), generator=g)
    assert len({int(Wt[0, 0, a, b]) for a in range(3) for b in range(3)}) > 2          # not symmetric: a flipped tap would show
    Y = R.y_from_weights(g_t, Wt)
    delta, _ = R.scatter_delta(rows, Y)
    auto = R.autograd_delta(rows, g_t, Wt)
    assert torch.equal(delta, auto) and float(delta.abs().max()) > 0
    flipped, _ = R.scatter_delta(rows, Y, sign=-1)
    assert not torch.equal(flipped, auto)
    # the opposite sign differs exactly on the targets whose neighbourhood is not point-symmetric in what reaches them: at least every
    # isolated pixel's ring, and never in the total (every contribution still lands somewhere unless it leaves the level)
    iso = R.row_of(0, 0, 5, 5)
    ring = [R.row_of(0, 0, 5 + a, 5 + b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
    assert torch.equal(flipped[iso], auto[iso]) and all(not torch.equal(flipped[t], auto[t]) for t in ring)


@pytest.mark.parametrize("Cf", [8, 24, 256, 2040, 2048])
def test_exact_case_operands_are_exact_in_every_dtype(Cf):
    rows = R.pixel_rows()
    cap = len(rows) + 4
    for Ty, Tm in ((torch.float32, torch.float32), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16)):
        Y, pre = R.y_exact(cap, len(rows), Cf, Ty), R.prefill_exact(Cf, Tm)
        assert torch.equal(Y.double(), R.y_exact(cap, len(rows), Cf, torch.float32).double()) and bool((Y[len(rows):] == 77).all())
        exact = pre.double() + R.scatter_delta(rows, Y)[0]
        assert torch.equal(exact, exact.round()) and float(exact.abs().max()) <= 256          # integers a bf16 holds exactly
        ref = R.scatter_ref(rows, Y, pre)
        assert ref.dtype == Tm and torch.equal(ref.double(), exact)
        assert torch.equal(R.scatter_ref(rows, Y, pre, round_each=True), ref)                 # nothing to round: the wrong variant agrees here
    assert len(set(Y[:len(rows)].flatten().tolist())) == 5


def test_single_rounding_case_has_both_ties_and_per_contribution_rounding_shows():
    rows = R.pixel_rows()
    cap, Cf = len(rows) + 4, 8
    Y, pre = R.y_ones(cap, len(rows), Cf), R.prefill_ties(Cf)
    assert torch.equal(pre.float().double(), (248 + torch.arange(Cf) % 4).double().repeat(R.TOTAL, 1))
    exact = pre.double() + R.scatter_delta(rows, Y)[0]
    ref = R.scatter_ref(rows, Y, pre)
    t = R.row_of(2, 0, 1, 1)                                            # an interior pixel of the fully active 3 x 4 level: nine contributions
    assert exact[t, :4].tolist() == [257.0, 258.0, 259.0, 260.0] and ref[t, :4].float().tolist() == [256.0, 258.0, 260.0, 260.0]
    inexact = ref.double() != exact
    assert int(inexact.sum()) > 0 and bool((exact[inexact] > 256).all())
    each = R.scatter_ref(rows, Y, pre, round_each=True)
    assert each[t, :4].float().tolist() == [256.0, 256.0, 256.0, 256.0]     # stuck at 256: 256 + 1 ties to even every time
    differs = (each.float() != ref.float()).any(dim=1)
    # per-contribution rounding differs exactly on targets whose exact result lies past 257 (where a bf16 step is 2)
    assert torch.equal(differs, (exact > 257).any(dim=1)) and int(differs.sum()) > 0


def test_gather_reference():
    rows = R.pixel_rows()
    cap, Cf = len(rows) + 5, 8
    for T in (torch.float32, torch.bfloat16):
        ghead = torch.randn(R.TOTAL, R.CH, generator=torch.Generator().manual_seed(1))
        hidden, feat = R.random_bits((R.TOTAL, Cf), T, 2), R.random_bits((R.TOTAL, Cf), T, 3)
        assert bool(feat.float().isnan().any()) and bool(hidden.float().isnan().any())          # NaN payloads are among the operands
        G, Tm, X9 = R.gather_ref(rows, cap, ghead, hidden, feat)
        assert G.dtype == Tm.dtype == X9.dtype == T and bool((R.as_int(X9[len(rows):]) == 0).all()) and bool((R.as_int(G[len(rows):]) == 0).all())
        s = rows.index(R.row_of(4, 1, 0, 0))                            # the 1 x 1 level: only the centre tap is inside
        assert torch.equal(R.as_int(X9[s, 4]), R.as_int(feat[rows[s]])) and int((R.as_int(X9[s]) != 0).any(dim=1).sum()) <= 1
        s = rows.index(R.row_of(0, 0, 0, 0))                            # top-left corner: taps 0, 1, 2, 3, 6 are outside
        assert all(bool((R.as_int(X9[s, tap]) == 0).all()) for tap in (0, 1, 2, 3, 6))
        assert torch.equal(R.as_int(X9[s, 8]), R.as_int(feat[R.row_of(0, 0, 1, 1)])) and torch.equal(R.as_int(X9[s, 5]), R.as_int(feat[R.row_of(0, 0, 0, 1)]))
        s = rows.index(R.row_of(0, 1, 0, 0))                            # image 1's first pixel does not see image 0's last row
        assert bool((R.as_int(X9[s, :3]) == 0).all())

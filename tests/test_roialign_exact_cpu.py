"""tests/roialign_exact.py pinned without a GPU: every lattice case meets its preconditions and its exactness budget, the case set holds
every edge the RoIAlign kernels branch on (asserted from the path facts of the reference's own sample walk), the oracle's fp32 roi_pool and
its autograd gradient equal the fp64 reference bit for bit on the lattice cases and stay within a derived fp32 bound on the random boxes,
and deliberately wrong variants of the reference differ from it exactly on the ROIs that carry the edge in question."""
import pytest
import torch

import roialign_exact as R


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _oracle(feats, rois, N, P, gp, dtype=torch.float32):
    """oracle.d2_rcnn.roi_pool and its autograd gradient, rows in the order of `rois`"""
    from oracle import d2_rcnn as d2
    order = torch.cat([(rois[:, 0] == i).nonzero().flatten() for i in range(N)])
    fr = [_nchw(f).to(dtype).requires_grad_(True) for f in feats]
    cfg = d2.make_cfg(num_classes=8)
    cfg["pooler_resolution"] = P
    out = d2.roi_pool(cfg, fr, [rois[rois[:, 0] == i, 1:] for i in range(N)])
    out.backward(_nchw(gp[order]).to(dtype))
    pooled = torch.empty_like(out)
    pooled[order] = out.detach()
    return pooled.permute(0, 2, 3, 1), [(f.grad if f.grad is not None else torch.zeros_like(f)).permute(0, 2, 3, 1) for f in fr]


# ================================================================================================ preconditions, budget, oracle
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_lattice_case_is_exact_and_the_oracle_equals_the_reference(name):
    c = R.cases()[name]
    assert c.N <= 4 and all(t.shape[3] == 256 for t in R.operands(name)[0])
    if name not in ("sep_208x8", "vec_209x8", "vec_2x345"):
        assert all(h <= 64 and w <= 70 for h, w in c.shapes)
    use_f, use_b = R.check_lattice(name)
    assert 0 < use_f < 1 and 0 < use_b < 1
    feats, gp = R.operands(name)
    out64, G64 = R.reference(name)
    # the oracle on the rows whose area is not negative (its level is undefined there); a padding row is not an oracle input at all
    area = (c.rois[:, 3] - c.rois[:, 1]) * (c.rois[:, 4] - c.rois[:, 2])
    keep = (area >= 0).nonzero().flatten()
    rois, gk = c.rois[keep], gp[keep]
    ref_rows = R.ref_forward(feats, rois, c.P)
    G_rows = R.ref_backward(c.shapes, c.N, rois, c.P, gk)
    if len(keep) == c.R and c.pad_at is None:
        assert torch.equal(ref_rows, out64)
    for a, b in zip(G_rows, G64):                       # the rows left out have no gradient
        assert torch.equal(a, b)
    pooled, grads = _oracle(feats, rois, c.N, c.P, gk)
    assert torch.equal(pooled.double(), ref_rows)
    for a, b in zip(grads, G_rows):
        assert torch.equal(a.double(), b)
    if c.pad_at is not None:                            # the padding row pools to zero, the rows around it are the rows of case.rois
        assert not out64[c.pad_at].any() and torch.equal(torch.cat([out64[:c.pad_at], out64[c.pad_at + 1:]]), R.ref_forward(feats, c.rois, c.P))


def test_random_boxes_oracle_is_within_an_fp32_bound_of_the_reference():
    """fp32 against fp64 on the same operands.  A coordinate is a handful of roundings at the magnitude cmax of the level coordinates:
    |dv| <= 8 * 2^-24 * cmax, which moves each of a sample's two fractions by as much; then 4 * count products and sums per element.
      forward   |err| <= 2^-24 * ((4 count + 8) * S + 32 cmax max|f|),      S = sum |w f| / count of the element
      backward  |err| <= 2^-24 * sum over ROIs ((4 count + 9) * A + 16 cmax max|g| * T),   A = sum |w g| / count, T = the ROI's samples with a tap on
                the pixel / count
    The measured error is far inside (printed); a wrong tap, clamp or level is of the order of max|f|."""
    b = R.bounded_case()
    u = 2.0 ** -24
    fmax, gmax = max(f.abs().max().item() for f in b["feats"]), b["gp"].abs().max().item()
    assert sorted(set(R.assign_levels(b["rois"]).tolist())) == [0, 1, 2, 3]
    assert any(f["x1"] < -1 or f["y1"] < -1 or f["x2"] > f["W"] or f["y2"] > f["H"] for f in b["facts"])
    assert {3, 5, 7} <= {f["gw"] for f in b["facts"]} | {f["gh"] for f in b["facts"]}
    bound_f = torch.zeros_like(b["out64"])
    bound_g = [torch.zeros(g.shape[:3], dtype=torch.float64) for g in b["G64"]]
    for r, f in enumerate(b["facts"]):
        cmax = max(abs(f[k]) for k in ("x1", "y1", "x2", "y2"))
        F = b["feats"][f["level"]][f["b"]].double().abs()
        S = torch.einsum("py,qx,yxc->pqc", f["RW"], f["CW"], F) / f["count"]
        bound_f[r] = u * ((4 * f["count"] + 8) * S + 32 * cmax * fmax)
        A = torch.einsum("py,qx,pq->yx", f["RW"], f["CW"], b["gp"][r].double().abs().amax(-1)) / f["count"]
        T = torch.einsum("py,qx->yx", f["RN"], f["CN"]) / f["count"]
        bound_g[f["level"]][f["b"]] += u * ((4 * f["count"] + 9) * A + 16 * cmax * gmax * T)
    ef = (b["out32"].double() - b["out64"]).abs()
    print(f"forward: max err {ef.max().item():.3e}, worst err / bound {(ef / bound_f).max().item():.3f}, max|ref| {b['out64'].abs().max().item():.3f}")
    assert bool((ef <= bound_f).all())
    for l in range(4):
        eg = (b["G32"][l].double() - b["G64"][l]).abs().amax(-1)
        ok = eg <= bound_g[l]
        print(f"level {l}: max err {eg.max().item():.3e}, worst err / bound {(eg / bound_g[l].clamp(min=1e-300)).max().item():.3f}, max|ref| {b['G64'][l].abs().max().item():.3f}")
        assert bool(ok.all())


# ================================================================================================ coverage
def _alive(f, axis):
    return [v for _, v, dead in f[axis] if not dead]


def _dead(f, axis):
    return [v for _, v, dead in f[axis] if dead]


def test_edges_case_holds_every_sampling_edge():
    c, fs = R.cases()["edges"], R.facts("edges")
    H, W = c.shapes[0]
    l0 = [f for f in fs if f["level"] == 0]
    for axis, size in (("ys", H), ("xs", W)):
        alive = [v for f in l0 for v in _alive(f, axis)]
        dead = [v for f in l0 for v in _dead(f, axis)]
        assert -1.0 in alive and float(size) in alive                       # exactly at -1 and at the size: alive
        assert -1.125 in dead and size + 0.125 in dead                      # one eighth beyond: dead
        assert 0.0 in alive and size - 1.0 in alive
        assert any(size - 1 < v < size for v in alive)                      # both taps on the last pixel
        assert any(v == int(v) and 0 < v < size - 1 for v in alive)         # weight exactly 0 on the high tap
        assert any(v - int(v) == 0.5 and 0 < v < size - 1 for v in alive)
    # over each corner (image 0 at the top left), entirely outside on each side, the whole map
    live = [f for f in fs if not f["zero"] and f["yext"][1] > f["yext"][0] and f["xext"][1] > f["xext"][0]]
    assert any(f["x1"] < -1 and f["y1"] < -1 and f["b"] == 0 and f["level"] == 0 for f in live)
    assert any(f["x2"] > f["W"] and f["y1"] < -1 for f in live) and any(f["x1"] < -1 and f["y2"] > f["H"] for f in live)
    assert any(f["x2"] > f["W"] and f["y2"] > f["H"] for f in live)
    out = [f for f in fs if not f["zero"] and f not in live]
    assert any(f["x2"] < -1 for f in out) and any(f["x1"] > f["W"] for f in out) and any(f["y2"] < -1 for f in out) and any(f["y1"] > f["H"] for f in out)
    assert all(not R.reference("edges")[0][fs.index(f)].any() for f in out)
    assert any(f["yext"] == (0, f["H"]) and f["xext"] == (0, f["W"]) and bool((f["RW"].sum(0) > 0).all()) and bool((f["CW"].sum(0) > 0).all()) for f in live)
    assert {f["level"] for f in live} == {0, 1, 2, 3} and {f["b"] for f in live} == {0, 1}
    # a dead bin column on the left of image 0, rows from row 0: where the separable forward used to read the pixel before the map
    assert any(f["b"] == 0 and f["fx"][0] == 0 and f["fy"][0] == 0 and f["col_runs"][0] == 0 and max(f["col_runs"]) > 0 for f in live)


def test_degenerate_case_holds_every_kind():
    c, fs = R.cases()["degenerate"], R.facts("degenerate")
    w, h = c.rois[:, 3] - c.rois[:, 1], c.rois[:, 4] - c.rois[:, 2]
    for cond in ((w == 0) & (h > 0), (h == 0) & (w > 0), (w < 0) & (h > 0), (w > 0) & (h < 0), (w < 0) & (h < 0), (w > 0) & (h > 0)):
        assert bool(cond.any())
    assert all(f["zero"] == bool(w[i] <= 0 or h[i] <= 0) for i, f in enumerate(fs))
    # negative width, positive height: the forward's footprint has a negative column count, rows from row 0 of image 0 among them
    neg = [f for i, f in enumerate(fs) if w[i] < 0 and h[i] > 0]
    assert any(f["fx"][1] - f["fx"][0] + 1 < -1 for f in neg) and any(f["fx"][1] - f["fx"][0] + 1 == -1 and f["fy"][0] == 0 and f["b"] == 0 for f in neg)
    fwd = c.forward_rois()
    assert len(fwd) == c.R + 1 and fwd[c.pad_at, 0] == -1 and (fwd[[c.pad_at - 1, c.pad_at + 1], 0] >= 0).all()
    assert R.facts("degenerate", True)[c.pad_at]["zero"]


def test_bin_geometry_and_pooling_sizes():
    fs = R.facts("bins")
    bins = {(f["x2"] - f["x1"]) / 7 for f in fs} | {(f["y2"] - f["y1"]) / 7 for f in fs}
    assert {0.25, 1.0, 1.5, 2.0, 3.5, 4.0, 7.5} <= bins
    rr = {v for f in fs for v in f["row_runs"].values()}
    assert max(rr) > 4 and {1, 2, 3, 4} <= rr                             # the gathers' extra bin-row loop: more than 3, more than 4
    quarter = [f for f in fs if (f["x2"] - f["x1"]) / 7 == 0.25]
    assert quarter and all(set(f["col_runs"]) <= {1, 2} for f in quarter)
    wm = {m for f in fs for m in f["wave_maxrun"]}
    assert {1, 2, 3, 4, 5, 6} <= wm and max(wm) >= 7                     # every exactly unrolled row loop of the separable forward, and the generic one
    assert any(max((f["x2"] - f["x1"]) / 7, 0) >= 7 and max(f["col_runs"]) >= 7 for f in fs)
    # P in {1, 2, 5, 7}: each with small and large bins, an overhanging ROI and every level
    for P in (1, 2, 5, 7):
        c, fm = R.cases()[f"mixed_P{P}"], R.facts(f"mixed_P{P}")
        assert c.P == P and {f["level"] for f in fm} == {0, 1, 2, 3}
        assert any(f["x1"] < -1 and f["y1"] < -1 and f["b"] == 0 for f in fm)
        assert {1, 2} <= {m for f in fm for m in f["wave_maxrun"]} and max(m for f in fm for m in f["wave_maxrun"]) >= 7
    assert max(v for f in R.facts("mixed_P7") for v in f["row_runs"].values()) > 4 and max(v for f in R.facts("mixed_P5") for v in f["row_runs"].values()) > 4


def test_map_shapes():
    for name in ("edges", "degenerate", "mixed_P5"):
        sh = R.cases()[name].shapes
        assert any(h % 2 for h, w in sh) and all(w % 32 for h, w in sh) and any(w < 32 for h, w in sh) and any(w > 64 for h, w in sh)
    f = R.facts("sep_208x8")[0]
    assert R.cases()["sep_208x8"].shapes[0] == (208, 8) and f["fy"] == (0, 207) and f["yext"] == (0, 208)     # the last shape the separable forward takes
    f = R.facts("vec_209x8")[0]
    assert R.cases()["vec_209x8"].shapes[0] == (209, 8) and f["fy"] == (0, 208) and f["yext"] == (0, 209)
    f = R.facts("vec_2x345")[0]
    assert R.cases()["vec_2x345"].shapes[0] == (2, 345) and f["fx"] == (0, 344) and f["xext"] == (0, 345)
    for name in ("sep_208x8", "vec_209x8", "vec_2x345"):
        assert all(f["level"] == 0 for f in R.facts(name))


def test_no_tap_reaches_the_margin_of_the_kernels_footprint():
    """The kernels' footprint is floor(a1) - 1 .. floor(a2) + 2 (clamped to the map).  A live sample lies in (a1, a2), so its taps lie in
    floor(a1) .. floor(a2) + 1: the outer row and column on either side never carry weight, in the lattice cases and on the random boxes.
    (Shrinking a gather's candidate test to floor(y2) + 1 therefore changes no value: no case can tell the two apart.)"""
    import math
    everything = [f for name in R.CASE_NAMES for f in R.facts(name)] + list(R.bounded_case()["facts"])
    n = 0
    for f in everything:
        for ext, a1, a2, size in ((f["yext"], f["y1"], f["y2"], f["H"]), (f["xext"], f["x1"], f["x2"], f["W"])):
            if ext[1] > ext[0]:
                n += 1
                assert ext[0] >= min(max(math.floor(a1), 0), size - 1) and ext[1] - 1 <= min(max(math.floor(a2) + 1, 0), size - 1)
    assert n > 300


def test_level_case_sits_on_the_thresholds():
    c, fs = R.cases()["levels"], R.facts("levels")
    b = c.rois[:, 1:].double()
    s = torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    for k, T in enumerate((112.0, 224.0, 448.0)):
        lo, at, hi = s[3 * k:3 * k + 3].tolist()
        assert at == T and abs((T - lo) / T - 2.0 ** -16) < 2.0 ** -30 and abs((hi - T) / T - 2.0 ** -16) < 2.0 ** -30
        assert [f["level"] for f in fs[3 * k:3 * k + 3]] == [k, k + 1, k + 1]
    out64, G64 = R.reference("levels")
    for r, f in enumerate(fs):                          # the pooled constant names the level, and only that level's map has a gradient
        vals = set(out64[r][out64[r] != 0].tolist())
        assert vals and all(v / (f["level"] + 1) in (0.5, 1.0) for v in vals), (r, vals)
    assert all(G64[l].any() for l in range(4))


def test_scan_case_candidate_counts():
    c = R.cases()["scan"]
    img = c.rois[:, 0]
    assert c.N == 4 and c.rois_sorted and bool((img[1:] >= img[:-1]).all())
    assert [int((img == i).sum()) for i in range(4)] == [0, 257, 0, 1]
    for rows in (1, 2):
        cnt = R.candidates(c.rois, c.shapes, c.N, c.P, rows, True)
        tot = cnt[0][1].sum(-1)
        have = set(tot.flatten().tolist())
        assert {0, 1, 2, 3} <= have and max(have) >= 5, (rows, have)
        assert bool(((cnt[0][1][..., 0] > 0) & (cnt[0][1][..., 1] > 0)).any())        # one segment fed by both 256-row chunks
        assert all(int(cnt[l][i].sum()) == 0 for l in range(4) for i in (0, 2)) and int(cnt[1][3].sum()) > 0
    G64 = R.reference("scan")[1]
    assert all(not G64[l][i].any() for l in range(4) for i in (0, 2)) and G64[0][1].any() and G64[1][3].any()


# ================================================================================================ wrong references
def _differs(name, mut):
    c = R.cases()[name]
    feats, _ = R.operands(name)
    good = R.ref_forward(feats, c.rois, c.P)
    bad = R.ref_forward(feats, c.rois, c.P, mut=mut)
    return {r for r in range(c.R) if not torch.equal(good[r], bad[r])}


def _weighted(fs):
    return {r for r, f in enumerate(fs) if not f["zero"] and f["yext"][1] > f["yext"][0] and f["xext"][1] > f["xext"][0]}


def test_wrong_references_differ_exactly_where_they_should():
    """the cases can see: a dead test with >= / <=, a missing clamp at H - 1, a dropped high tap, a footprint one row short, a level
    threshold shifted by one"""
    fs = R.facts("edges")
    live = _weighted(fs)

    def has(r, pred):
        f = fs[r]
        return any(pred(v, f["H"]) for v in _alive(f, "ys")) or any(pred(v, f["W"]) for v in _alive(f, "xs"))
    # dead test: the ROIs with a live sample exactly at -1 or exactly at the size, and no other
    assert _differs("edges", "dead_ge") == {r for r in live if has(r, lambda v, n: v == -1.0 or v == n)} != set()
    # clamp: the ROIs with a live sample in (size - 1, size]
    assert _differs("edges", "no_clamp") == {r for r in live if has(r, lambda v, n: n - 1 < v <= n)} != set()
    # high tap: the ROIs with a live sample that has a fraction (after the clamps)
    assert _differs("edges", "no_hi") == {r for r in live if has(r, lambda v, n: 0 < v < n - 1 and v != int(v))} != set()
    # the last row with weight dropped / the next level: every ROI with weight (the coarsest level has no next one)
    assert _differs("edges", "short") == live
    assert {r for r in live if fs[r]["level"] < 3} <= _differs("edges", "level") <= {r for r in range(len(fs)) if fs[r]["level"] < 3}
    assert _differs("levels", "level") == {r for r, f in enumerate(R.facts("levels")) if f["level"] < 3}
    for mut in R.MUTANTS:
        assert _differs("mixed_P5", mut) and _differs("mixed_P1", mut), mut

"""Pins label_pipeline_refs.py without a GPU: the two matcher references (oracle fp32, integer) agree on every scene in both layouts, every
scene carries the edge it is named for (asserted on the operands, not assumed), the threshold neighbours fall on the recorded side, the
model of the dispatch names every arm, and deliberately wrong variants of the references differ from them exactly where the edge is."""
import numpy as np
import pytest
import torch

import label_pipeline_refs as R


def _cases():
    return [(name, big) for name in R.SCENES for big in (False, True)]


@pytest.mark.parametrize("name,big", _cases())
def test_oracle_and_integer_matchers_agree(name, big):
    sc = R.scene(name)
    for cfg in sc.configs:
        ints, orcs = R.references(name, big, cfg)
        assert len(ints) == sc.N
        for a, b in zip(ints, orcs):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x, y)


def test_thresholds_are_exact_quotients_and_the_oracle_takes_them_as_the_issue_states():
    from oracle import d2_rcnn as d2
    assert R.f32_of_fraction(3, 10) == np.float32(0.3) and R.f32_of_fraction(7, 10) == np.float32(0.7) and R.f32_of_fraction(1, 2) == np.float32(0.5)
    q = torch.tensor([[3.0], [7.0], [1.0]]) / torch.tensor([[10.0], [10.0], [2.0]])          # fp32 quotients, one GT x one box each
    labs = [int(d2.matcher(q[i:i + 1], [0.3, 0.7], [0, -1, 1], False)[1][0]) for i in range(3)]
    assert labs == [-1, 1, -1]
    assert int(d2.matcher(q[2:3], [0.5], [0, 1], False)[1][0]) == 1


def test_threshold_neighbours_fall_on_the_recorded_side():
    for num, den, thr in R.THRESHOLDS:
        below, above = R.nearest_quotients(num, den)
        assert below[0] * den < num * below[1] and above[0] * den > num * above[1]          # strictly below / above as exact quotients
        for p, u in (below, above):
            assert 0 < p < u and p + u < R.LIM
        sides = (R.side(*below, thr), R.side(*above, thr))
        print(f"{num}/{den}: below {below[0]}/{below[1]} -> {sides[0]}, above {above[0]}/{above[1]} -> {sides[1]}   "
              f"(fp32 bits {R.f32_of_fraction(*below).view(np.uint32):#x} | {np.float32(thr).view(np.uint32):#x} | {R.f32_of_fraction(*above).view(np.uint32):#x})")
        assert sides == R.NEIGHBOUR_SIDES[f"{num}/{den}"]
        # exhaustive as claimed: nothing closer among ALL admissible denominators near the bound, nor with a smaller one far from it
        for u in list(range(below[1] + 1, below[1] + 40)) + [below[1] // 2, below[1] // 3]:
            for p in ((num * u - 1) // den, num * u // den + 1):
                if 0 < p < u and p + u < R.LIM and p * den != num * u:
                    d = abs(num * u - den * p) * (below[1] if p * den < num * u else above[1])
                    ref = abs(num * below[1] - den * below[0]) * u if p * den < num * u else abs(num * above[1] - den * above[0]) * u
                    assert d >= ref


def test_threshold_scene_labels_follow_the_side():
    sc = R.scene("threshold")
    (rpn_on,), _ = R.references("threshold", False, (0.3, 0.7, True))
    (rpn_off,), _ = R.references("threshold", False, (0.3, 0.7, False))
    (single,), _ = R.references("threshold", False, (0.5, 0.5, False))
    for k, (name, tag, p, u, thr) in enumerate(sc.facts["pairs"]):
        s = "eq" if tag == "exact" else R.NEIGHBOUR_SIDES[name][0 if tag == "below" else 1]
        assert rpn_off[0][k].numpy() == R.f32_of_fraction(p, u) and int(rpn_off[1][k]) == k
        want = {0.3: {"lt": 0, "eq": -1, "gt": -1}, 0.7: {"lt": -1, "eq": 1, "gt": 1}, 0.5: {"lt": -1, "eq": -1, "gt": -1}}[thr][s]
        assert int(rpn_off[2][k]) == want, (name, tag)
        assert int(rpn_on[2][k]) == want, "the champions keep the low-quality rule off the boxes under test"
        if thr == 0.5:
            assert int(single[2][k]) == {"lt": 0, "eq": 1, "gt": 1}[s]
    for k, thr in zip((9, 10, 11), (0.3, 0.7, 0.5)):                 # the pairs that are not nested
        assert rpn_off[0][k].numpy() == np.float32(thr)


def test_ties_scene_has_the_ties_and_the_lower_index_wins():
    sc = R.scene("ties")
    boxes, L, _ = R.layout(sc, False)
    gt, gcnt = R.gt_tensor(sc)
    for n, w in enumerate(sc.facts["where"]):
        iou = R.int_iou(gt[n, :gcnt[n]], boxes[n])
        (d0, d1), (e0, e1) = w["dup"], w["eq"]
        assert torch.equal(gt[n, d0], gt[n, d1]) and not torch.equal(gt[n, e0], gt[n, e1])
        assert iou[d0, 0] == iou[d1, 0] == iou[:, 0].max() and iou[e0, 1] == iou[e1, 1] == iou[:, 1].max()
        ref = R.references("ties", False, (0.3, 0.7, False))[0][n]
        assert int(ref[1][0]) == d0 and int(ref[1][1]) == e0
        # all 16 GTs meet both workgroups' union boxes: the four quarters of the parts == 4 kernel are 0-3, 4-7, 8-11, 12-15
        assert all(len(lst) == 16 for lst in R.cull_lists(gt[n, :gcnt[n]], boxes[n], L, L))
    q = lambda i: i // 4
    w0, w1 = sc.facts["where"]
    assert q(w0["dup"][0]) == q(w0["dup"][1]) and q(w0["eq"][0]) == q(w0["eq"][1])
    assert q(w1["dup"][0]) != q(w1["dup"][1]) and q(w1["eq"][0]) != q(w1["eq"][1])


def test_tiles_scene_crosses_the_256_tile():
    sc = R.scene("tiles")
    boxes, L, _ = R.layout(sc, False)
    gt, gcnt = R.gt_tensor(sc)
    assert gcnt == [257, 300] and sc.gmax == 300
    refs = R.references("tiles", False, (0.3, 0.7, False))[0]

    def at(box):
        return int((boxes[0] == torch.tensor(box)).all(dim=1).nonzero()[0])
    shifted = lambda k: (R._grid_gt(k)[0] + 2, R._grid_gt(k)[1], R._grid_gt(k)[2] + 2, R._grid_gt(k)[3])
    for k in (256, 259, 299):
        assert int(refs[1][1][at(shifted(k))]) == (k if k != 259 else 0)          # image 1: GT 259 was moved onto GT 3
    assert int(refs[0][1][at(shifted(256))]) == 256 and float(refs[0][0][at(shifted(299))]) == 0.0 and int(refs[0][1][at(shifted(299))]) == 0
    both = at((R._grid_gt(255)[0], R._grid_gt(255)[1], R._grid_gt(256)[2], R._grid_gt(256)[3]))
    iou = R.int_iou(gt[1], boxes[1])
    assert iou[255, both] == iou[256, both] == iou[:, both].max() > 0 and int(refs[1][1][both]) == 255
    i3 = at(shifted(3))
    assert torch.equal(gt[1, 3], gt[1, 259]) and iou[3, i3] == iou[259, i3] == iou[:, i3].max() and int(refs[1][1][i3]) == 3


def test_low_quality_scene():
    sc = R.scene("low_quality")
    on, off = R.references("low_quality", False, (0.3, 0.7, True))[0], R.references("low_quality", False, (0.3, 0.7, False))[0]
    gt, gcnt = R.gt_tensor(sc)
    assert gcnt == [1, sc.gmax, 0, 3, sc.gmax]
    three = list(sc.facts["three"])
    assert all(float(v) == np.float32(0.1) for v in on[0][0][three]) and on[0][2][three].tolist() == [1, 1, 1] and off[0][2][three].tolist() == [0, 0, 0]
    assert int(on[0][2].sum()) == 3 + 60                               # (and the 60 copies of box 0 that pad its wave of 4 boxes)
    for n in sc.facts["claims_all"]:
        assert bool((on[n][2] == 1).all()) and not bool((off[n][2] == 1).all())
    n = sc.facts["no_gt"]
    assert bool((on[n][2] == 0).all()) and bool((on[n][1] == 0).all())
    zero_area = gt[3, 2]
    assert int(R.int_area(zero_area[None])[0]) == 0 and int(R.int_iou(gt[3, :3], R.layout(sc, False)[0][3])[2].count_nonzero()) == 0
    assert 0 < int((on[4][2] == 1).sum()) < on[4][2].numel() and not torch.equal(on[4][2], off[4][2])


@pytest.mark.parametrize("big", [False, True])
def test_culling_scene_and_the_culled_matcher(big):
    sc = R.scene("culling")
    boxes, L, pos = R.layout(sc, big)
    gt, gcnt = R.gt_tensor(sc)
    g, b, f = gt[0, :gcnt[0]], boxes[0], sc.facts
    lists = R.cull_lists(g, b, L, L)
    inter = R.int_inter_union(g, b)[0]
    wave = lambda k: slice(pos[k], pos[k] + 64)
    grp, k = f["gap"]
    assert k in lists[pos[grp] // 64] and int(inter[k, wave(grp)].sum()) == 0                    # meets the union, no box
    grp, k = f["edge"]
    assert k not in lists[pos[grp] // 64] and int(g[k, 0]) == int(b[wave(grp), 2].max())         # shares the edge, is not listed
    grp, k = f["clusters"]
    assert k in lists[pos[grp] // 64] and int(inter[k, wave(grp)].sum()) == 0
    assert int(b[wave(grp), 0].max()) - int(b[wave(grp), 0].min()) >= 2000
    assert L - pos[-1] == R.BIG_TAIL and int(b[pos[-1]:, :2].min()) >= 100                      # the ragged wave: far from the origin
    assert f["origin"] not in lists[-1] and g[f["origin"], :2].tolist() == [0, 0]
    assert inter[f["last_only"]].nonzero().flatten().tolist() == [L - 1]                        # only the last active box
    # the wrong variant (inactive lanes widen the union): only the ragged wave's list changes; it gains the GT at the origin (and those
    # between the origin and the wave's boxes) and loses nothing
    wide = R.cull_lists(g, b, L, L, widen_inactive=True)
    assert wide[:-1] == lists[:-1] and set(lists[-1]) < set(wide[-1]) and f["origin"] in wide[-1]
    for cfg in sc.configs:
        for group in (64, 256, 1024):
            ref = R.references("culling", big, cfg)[0][0]
            got = R.culled_match(g, b, L, L, *cfg, group=group)
            assert all(torch.equal(x, y) for x, y in zip(got, ref))


@pytest.mark.parametrize("name", [n for n in R.SCENES if n != "culling"])
def test_culling_is_sound_on_every_scene(name):
    """the kernels' way (per-group lists, running maximum from (0, index 0), the zero-best flag) == the plain reference"""
    sc = R.scene(name)
    boxes, L, _ = R.layout(sc, False)
    gt, gcnt = R.gt_tensor(sc)
    for cfg in sc.configs:
        for n, cnt in enumerate(R.box_counts(sc, L)):
            ref = R.references(name, False, cfg)[0][n]
            for group in (64, 256):
                got = R.culled_match(gt[n, :gcnt[n]], boxes[n], cnt, L, *cfg, group=group)
                assert all(torch.equal(x, y) for x, y in zip(got, ref)), (name, cfg, n, group)


def test_counts_scene():
    sc = R.scene("counts")
    boxes, L, cnt, gt, gcnt = R.operands(sc, False)
    assert cnt == [L - 5, 0, 70] and boxes.shape[1] == L + 3 and L % 64 != 0
    for n in range(sc.N):
        assert bool((boxes[n, cnt[n]:] == gt[n, 0]).all())            # what a read past the count would see: IoU 1 with GT 0
    assert R.box_counts(sc, R.BIG_L) == [R.BIG_L - 5, 0, 70]


def test_every_arm_of_the_dispatch_is_named_and_reached():
    for name in R.SCENES:
        sc = R.scene(name)
        arms = R.arms_for(sc)
        assert len(arms) == 5 and ("wg64" in arms) == (sc.gmax > 256)
        for arm in arms:
            big, padded, mw = R.ARMS[arm]
            L = R.layout(sc, big)[1]
            assert (L * sc.N >= 65536) == big
            words = sc.N * sc.gmax * (32 if padded else 1)
            for knob in ((0, 1) if mw is None else (mw,)):
                assert R.select_arm(L, sc.N, sc.gmax, 4 * words, knob) == arm
    assert {a for n in R.SCENES for a in R.arms_for(R.scene(n))} == set(R.ARMS)
    assert R.BIG_L > 65536 and R.BIG_L % 64 == R.BIG_TAIL == 37


# ------------------------------------------------------------------------------------------------
# wrong variants of the matcher reference differ exactly at the edge
# ------------------------------------------------------------------------------------------------
def _per_image(name):
    sc = R.scene(name)
    boxes, L, _ = R.layout(sc, False)
    gt, gcnt = R.gt_tensor(sc)
    for n, cnt in enumerate(R.box_counts(sc, L)):
        if cnt and gcnt[n]:
            yield n, gt[n, :gcnt[n]], boxes[n, :cnt]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_last_maximum_differs_exactly_where_the_maximum_is_not_unique(name):
    found = 0
    for n, g, b in _per_image(name):
        ref, bad = R.int_match(g, b, 0.3, 0.7, False), R.int_match(g, b, 0.3, 0.7, False, last_max=True)
        iou = R.int_iou(g, b)
        multiple = (iou == iou.max(dim=0).values[None]).sum(dim=0) > 1           # (a box no GT overlaps ties all of them at 0: index 0)
        assert torch.equal(ref[1] != bad[1], multiple) and torch.equal(ref[0], bad[0])
        found += int((multiple & (ref[0] > 0)).sum())
    assert (found > 0) == (name in ("ties", "tiles"))


@pytest.mark.parametrize("name", list(R.SCENES))
def test_strict_comparison_differs_exactly_on_the_threshold(name):
    sc, found = R.scene(name), 0
    for n, g, b in _per_image(name):
        for lo, hi, _ in sc.configs:
            ref, bad = R.int_match(g, b, lo, hi, False), R.int_match(g, b, lo, hi, False, strict_ge=True)
            on = (ref[0] == torch.tensor(lo, dtype=torch.float32)) | (ref[0] == torch.tensor(hi, dtype=torch.float32))
            assert torch.equal(ref[2] != bad[2], on)
            found += int(on.sum())
    assert (found > 0) == (name == "threshold")


@pytest.mark.parametrize("name", list(R.SCENES))
def test_low_quality_rule_with_overlap_only_differs_exactly_where_a_gt_has_no_overlap(name):
    differing = []
    for n, g, b in _per_image(name):
        ref, bad = R.int_match(g, b, 0.3, 0.7, True), R.int_match(g, b, 0.3, 0.7, True, lowq_needs_overlap=True)
        zero_best = bool((R.int_iou(g, b).max(dim=1).values == 0).any())
        assert (not torch.equal(ref[2], bad[2])) == zero_best
        if zero_best:
            assert bool((ref[2] == 1).all())
            differing.append(n)
    assert differing == (list(R.scene("low_quality").facts["claims_all"]) if name == "low_quality" else [])


# ------------------------------------------------------------------------------------------------
# B: lists, ROI preparation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg,K", [(0, 1), (8, 8)])
def test_label_patterns_and_their_lists(bg, K):
    L = 3 * 4096 + 5
    want = {"all_pos": (L, 0), "all_bg": (0, L), "all_ignore": (0, 0), "all_pad": (0, 0), "alternating": ((L + 1) // 2, L // 2),
            "first_only": (1, 0), "last_only": (0, 1), "segment_firsts": (2, 2)}
    assert set(want) == set(R.LABEL_PATTERNS)
    for kind, (npos, nneg) in want.items():
        lab = R.label_pattern(kind, L, bg, K)
        pos, neg = R.compact_ref(lab, bg)
        assert lab.dtype == torch.int32 and (pos.numel(), neg.numel()) == (npos, nneg), kind
        assert bool((pos[1:] > pos[:-1]).all()) and bool((neg[1:] > neg[:-1]).all())
    assert R.COMPACT_L[-1] == 65 * 4096 + 1 == 266241 and -(-R.COMPACT_L[-1] // 4096) == 66          # 65 earlier segments: a second round of 64


@pytest.mark.parametrize("P,Gmax", [(13, 1), (37, 256), (251, 6)])
def test_roi_reference_is_the_oracles_labelling(P, Gmax):
    from oracle import d2_rcnn as d2
    sc = R.roi_scene(P, Gmax)
    assert (P + Gmax) % 8 != 0 and (P + Gmax) % 256 != 0
    ref = R.roi_prepare_ref(sc)
    cfg = dict(num_classes=sc["K"], roi_iou_threshold=0.5, roi_batch_per_image=1 << 20, roi_positive_fraction=0.5)
    props = [dict(proposal_boxes=sc["props"][n, :sc["pcount"][n]].float(), image_size=(400, 400)) for n in range(sc["N"])]
    tgts = [dict(gt_boxes=sc["gt"][n, :sc["gcount"][n]].float(), gt_classes=sc["gcls"][n, :sc["gcount"][n]]) for n in range(sc["N"])]
    full = d2.label_and_sample_proposals(cfg, props, tgts)            # a batch that large keeps every candidate: the draw only permutes
    for n, (r, o) in enumerate(zip(ref, full)):
        nf = r["fg"].numel()
        assert sorted(o["sampled_idxs"][:nf].tolist()) == r["fg"].tolist() and sorted(o["sampled_idxs"][nf:].tolist()) == r["bg"].tolist()
        assert torch.equal(o["gt_classes"], r["cls"][o["sampled_idxs"]])
        assert r["count"] == sc["pcount"][n] + sc["gcount"][n] == r["fg"].numel() + r["bg"].numel()
        gc = sc["gcount"][n]
        if gc and r["count"]:                                         # and the integer reference agrees with it
            cand = torch.cat([sc["props"][n, :sc["pcount"][n]], sc["gt"][n, :gc]])
            R.assert_lattice(sc["gt"][n, :gc], cand)
            b, i, lab = R.int_match(sc["gt"][n, :gc], cand, 0.5, 0.5, False)
            assert torch.equal(b, r["best"]) and torch.equal(i, r["midx"]) and torch.equal(lab, r["lab"])
        else:
            assert bool((r["cls"] == sc["K"]).all())
    r0 = ref[0]
    assert float(r0["best"][0]) == 1.0 and float(r0["best"][1]) == 0.5 and float(r0["best"][2]) == np.float32(0.4)
    assert r0["lab"][:3].tolist() == [1, 1, 0] and r0["midx"][:2].tolist() == [0, 0] and int(r0["cls"][0]) == int(sc["gcls"][0, 0])
    assert ref[1]["count"] == sc["gcount"][1] > 0 and ref[2]["fg"].numel() == 0 and ref[3]["count"] == 0

"""Directed edge cases of the discrete post-processing path -- candidate filter and sort, NMS suppression mask, greedy NMS scan,
top-k / pseudo-label compaction (csrc/nms.h, the det_* kernels of csrc/roi.hip, the topk_* / rpn_merge kernels of csrc/rpn.hip) -- against
the CPU oracle (oracle.d2_rcnn.fast_rcnn_inference / find_top_rpn_proposals, oracle.aldi_ops.process_bbox).  Random scenes give suppression
chains a handful deep and never an empty list; the scenes here are built so that a wrong keep or drop changes an exact order or count.

Every scene's expectation is computed by the oracle at run time; the survivor counts the scenes were designed for are asserted on the oracle's
side as well.  Every detection scene runs under both NMS-mask kernels (knob nms_mask_tri), every RPN scene additionally under both top-k forms
(knob rpn_topk_fused); all arms must agree bit for bit in every output tensor.  Tolerances are the neighbouring tests' (test_kernels_gpu.py):
1e-6 on detection scores, 1e-3 on boxes, RPN scores bit-exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, CP, TOPK = 8, 48, 100
SENTINEL = -7.0


@pytest.fixture(autouse=True)
def _reset_tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _cfg(**over):
    from oracle import d2_rcnn as d2
    return d2.make_cfg(num_classes=K, **over)


def _rand_boxes(n, w, h, g, lo=4.0, hi=120.0):
    x1 = torch.rand(n, generator=g) * (w - lo)
    y1 = torch.rand(n, generator=g) * (h - lo)
    bw = lo + torch.rand(n, generator=g) * (hi - lo)
    bh = lo + torch.rand(n, generator=g) * (hi - lo)
    return torch.stack([x1, y1, (x1 + bw).clamp(max=w), (y1 + bh).clamp(max=h)], 1)


# ------------------------------------------------------------------------------------------------
# detection path: scene builders (CPU), the oracle, the device call, the comparison
# ------------------------------------------------------------------------------------------------
def _single_rows(classes, logits):
    """rows that are one candidate each: logit[class] = a, background (the LAST of the K + 1) = 0, every other logit -30, deltas 0:
    score = softmax = sigmoid(a) up to 7 e^-30, decoded box = the proposal"""
    logits = torch.as_tensor(logits, dtype=torch.float32)
    R = len(logits)
    pred = torch.zeros(R, CP)
    pred[:, :K] = -30.0
    pred[torch.arange(R), torch.as_tensor(classes)] = logits
    return pred


def _random_image(P, g, scale=1.5, size=(200, 300)):
    """the recipe of test_detections_and_pseudolabel_filter_vs_oracle, with logits of half its spread: the best scores stay away from 1, where
    fp32 scores crowd within an ulp of each other and the expected order would rest on the last bit of expf"""
    pred = torch.randn(P, CP, generator=g)
    pred[:, : K + 1] *= scale
    pred[:, K + 1:] *= 0.5
    return _rand_boxes(P, size[1], size[0], g, lo=8, hi=150), pred


def _scene(images):
    """images: list of (props (p, 4), pred (p, CP), (h, w)); batch arrays of P = the longest list + 5 rows (the rows beyond an image's count
    hold values that would be candidates if a kernel read them)"""
    N = len(images)
    P = max(len(b) for b, _, _ in images) + 5
    props = torch.zeros(N, P, 4)
    props[:, :, 2:] = 9.0
    pred = torch.zeros(N, P, CP)
    pred[:, :, 0] = 8.0
    for n, (b, p, _) in enumerate(images):
        props[n, : len(b)] = b
        pred[n, : len(b)] = p
    return dict(props=props, pred=pred, pcount=[len(b) for b, _, _ in images], sizes=[tuple(s) for _, _, s in images], N=N, P=P)


def _oracle_det(sc, topk=TOPK):
    from oracle import d2_rcnn as d2
    proposals = [{"proposal_boxes": sc["props"][n, :c], "image_size": sc["sizes"][n]} for n, c in enumerate(sc["pcount"])]
    rows = torch.cat([sc["pred"][n, :c] for n, c in enumerate(sc["pcount"])])
    return d2.fast_rcnn_inference(_cfg(detections_per_image=topk), rows[:, : K + 1], rows[:, K + 1: K + 1 + 4 * K], proposals)


def _oracle_candidates(sc, n):
    """what the oracle's score filter lets through for image n (non-finite rows dropped first, as fast_rcnn_inference does)"""
    pr = torch.softmax(sc["pred"][n, : sc["pcount"][n], : K + 1], dim=-1)
    pr = pr[torch.isfinite(pr).all(dim=1)]
    return int((pr[:, :K] > 0.05).sum())


_WS = {}


def _det_workspace(N):
    from aldi_amd import ops
    if N not in _WS:
        _WS[N] = torch.empty(ops.detections_workspace(N), dtype=torch.uint8, device=DEV)
    return _WS[N]


def _run_det(sc, pl_thresh, tri, topk=TOPK, pl_rows=None):
    """one aldi_detections call; every output buffer starts from a sentinel and comes back whole"""
    from aldi_amd import _lib as L
    from aldi_amd import ops
    from aldi_amd.engine import ROI_WEIGHTS
    L.reset_tuning()
    L.set_tuning("nms_mask_tri", tri)
    N, P = sc["N"], sc["P"]
    pl_rows = topk if pl_rows is None else pl_rows
    i32 = torch.int32
    out = dict(db=torch.full((N, topk, 4), SENTINEL, device=DEV), ds=torch.full((N, topk), SENTINEL, device=DEV),
               dc=torch.full((N, topk), int(SENTINEL), dtype=i32, device=DEV), dcount=torch.full((N,), int(SENTINEL), dtype=i32, device=DEV),
               pb=torch.full((N, pl_rows, 4), SENTINEL, device=DEV), pc=torch.full((N, pl_rows), int(SENTINEL), dtype=i32, device=DEV),
               ps=torch.full((N, pl_rows), SENTINEL, device=DEV), pl_count=torch.full((N,), int(SENTINEL), dtype=i32, device=DEV),
               err=torch.zeros(1, dtype=i32, device=DEV))
    ops.detections(sc["pred"].view(N * P, CP).to(DEV), CP, K, sc["props"].to(DEV), torch.tensor(sc["pcount"], dtype=i32, device=DEV), P, N,
                   torch.tensor(sc["sizes"], dtype=i32, device=DEV), ROI_WEIGHTS, 0.05, 0.5, topk, pl_thresh, _det_workspace(N),
                   out["db"], out["ds"], out["dc"], out["dcount"], out["pb"], out["pc"], out["ps"], out["pl_count"], out["err"])
    torch.cuda.synchronize()
    L.reset_tuning()
    return {k: v.cpu() for k, v in out.items()}


def _run_det_arms(sc, pl_thresh, **kw):
    """both NMS-mask kernels: identical bits in every output tensor (NaN cannot occur: checked finite)"""
    a, b = _run_det(sc, pl_thresh, 1, **kw), _run_det(sc, pl_thresh, 0, **kw)
    for k in a:
        assert bool(torch.isfinite(a[k].float()).all()), k
        assert torch.equal(a[k], b[k]), ("nms_mask_tri 1 vs 0", k)
    return a


def _check_image(out, n, ref, pl_thresh, topk=TOPK):
    """image n against the oracle: count, exact order and classes, scores, boxes, the unused rows, the pseudo-labels and their unused rows"""
    from oracle import aldi_ops as ao
    k = int(out["dcount"][n])
    assert k == len(ref["scores"]), (n, k, len(ref["scores"]))
    assert torch.equal(out["dc"][n, :k].long(), ref["pred_classes"]), n
    if k:
        assert float((out["ds"][n, :k] - ref["scores"]).abs().max()) < 1e-6, n
        assert float((out["db"][n, :k] - ref["pred_boxes"]).abs().max()) < 1e-3, n
    assert bool((out["db"][n, k:] == 0).all()) and bool((out["ds"][n, k:] == 0).all()) and bool((out["dc"][n, k:] == -1).all()), n
    pl = ao.process_bbox(ref, pl_thresh)
    m = int(out["pl_count"][n])
    assert m == len(pl["scores"]), (n, m, len(pl["scores"]))
    assert torch.equal(out["pc"][n, :m].long(), pl["gt_classes"]), n
    if m:
        assert float((out["ps"][n, :m] - pl["scores"]).abs().max()) < 1e-6, n
        assert float((out["pb"][n, :m] - pl["gt_boxes"]).abs().max()) < 1e-3, n
        assert bool((out["ps"][n, :m] > pl_thresh).all()), n
    rows = out["pc"].shape[1]
    j = torch.arange(m, rows)
    assert bool((out["pb"][n, m:] == 0).all()) and bool((out["ps"][n, m:] == 0).all()), n
    assert torch.equal(out["pc"][n, m:].long(), torch.where(j < topk, -1, 0)), n            # class -1 up to topk, 0 beyond
    return k, m


def _well_posed(ref):
    """the expected ORDER must not rest on a tie rule or on the last ulp of expf: the oracle's kept scores are strictly decreasing with gaps
    far above the 1e-7 by which the device's softmax may differ"""
    s = ref["scores"]
    return len(s) < 2 or float((s[:-1] - s[1:]).min()) > 1e-6


def _chain_image(n, s):
    i = torch.arange(n, dtype=torch.float32)
    boxes = torch.stack([i * s, torch.zeros(n), i * s + 10.0, torch.full((n,), 10.0)], 1)
    return boxes, _single_rows([2] * n, torch.linspace(6.0, 0.5, n)), (20, int(n * s + 20))


# ---- A1: successor chains
@pytest.mark.parametrize("n,s,survivors,stride", [(150, 2.0, 75, 2), (300, 2.0, 100, 2), (200, 1.0, 50, 4), (130, 3.0, 65, 2)])
def test_det_successor_chain(n, s, survivors, stride):
    """boxes [i s, 0, i s + 10, 10] in score order: every box suppresses only its successor(s), so a 64-box chunk of the scan needs one
    fixed-point round per box and the first box of a chunk depends on every earlier chunk; the chain is image 1 of the batch, image 0 a
    random scene with another row count (a wrong batch stride shows).  n = 300 cuts at topk in the middle of chunk 3 with survivors left
    in chunk 4."""
    g = torch.Generator().manual_seed(300 + n)
    rb, rp = _random_image(640, g)
    sc = _scene([(rb, rp, (200, 300)), _chain_image(n, s)])
    ref = _oracle_det(sc)
    thr = 0.982                                                  # sigmoid(4): inside every chain's score range, also of the first 100 of n = 300
    # the oracle's side of the scene: the designed survivor count, the designed survivors, strictly decreasing scores
    assert len(ref[1]["scores"]) == survivors
    assert torch.equal(ref[1]["pred_boxes"][:, 0], torch.arange(survivors, dtype=torch.float32) * stride * s)
    assert _well_posed(ref[0]) and _well_posed(ref[1]) and len(ref[0]["scores"]) == TOPK
    out = _run_det_arms(sc, thr)
    assert int(out["err"]) == 0
    for i in range(2):
        _check_image(out, i, ref[i], thr)
    assert 0 < int(out["pl_count"][1]) < int(out["dcount"][1])


def test_det_successor_chain_4200_boxes():
    """the one large scene: 4200 chained boxes (the sort at 8192 keys, 66 scan chunks, the <8,16> scan instance with mask rows 128 words
    wide).  With topk = 100 the scan stops in chunk 3; the same scene with topk = 2200 -- more than its 2100 survivors -- makes the scan walk
    all 66 chunks with a full-depth chain in each, every one depending on all chunks before it."""
    g = torch.Generator().manual_seed(42)
    rb, rp = _random_image(640, g)
    # (beside the chain: a random scene at topk = 100; at topk = 2200 a random scene's own 1000+ low-score detections would rest on
    # last-ulp score differences, so the neighbour is a directed scene there)
    for topk, survivors, other in ((TOPK, 100, (rb, rp, (200, 300))), (2200, 2100, _five_proposals())):
        sc = _scene([_chain_image(4200, 2.0), other])
        assert sc["P"] >= 4200 and _oracle_candidates(sc, 0) == 4200
        ref = _oracle_det(sc, topk)
        assert len(ref[0]["scores"]) == survivors and _well_posed(ref[0]) and _well_posed(ref[1])
        assert torch.equal(ref[0]["pred_boxes"][:, 0], torch.arange(survivors, dtype=torch.float32) * 4.0)
        thr = 0.5 * float(ref[0]["scores"][40] + ref[0]["scores"][41])            # between two kept scores 6e-6 apart: 41 pseudo-labels
        out = _run_det_arms(sc, thr, topk=topk)
        assert int(out["err"]) == 0
        for i in range(2):
            _check_image(out, i, ref[i], thr, topk=topk)
        assert int(out["pl_count"][0]) == 41


# ---- A2: the bitonic sort's sizes
def _scale_for_count(base, target):
    """logit scale at which the oracle's score filter lets `target` +- 2 candidates through, none of them within 1e-6 of the threshold (so the
    device, whose expf may differ in the last ulp, counts the same)"""
    def stats(scale):
        pr = torch.softmax(base[:, : K + 1] * scale, dim=-1)[:, :K]
        return int((pr > 0.05).sum()), float((pr - 0.05).abs().min())
    lo, hi = 0.25, 16.0                                          # the count falls as the scale grows
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        c, margin = stats(mid)
        if abs(c - target) <= 2 and margin > 1e-6:
            return mid, c
        if c > target:
            lo = mid
        else:
            hi = mid
    raise AssertionError(f"no logit scale gives {target} candidates")


@pytest.mark.parametrize("bound,seed", [(1024, 1024), (2048, 2048), (4096, 4098)])
def test_det_sort_sizes(bound, seed):
    """candidate counts just below (image 0) and just above (image 1) a power of two: the sort runs at `bound` and at 2 x `bound` keys"""
    g = torch.Generator().manual_seed(seed)                      # (seeds whose 100 best scores lie > 1e-5 apart: see _well_posed)
    P = bound // 4                                               # ~4 candidates per row: a logit scale near 1.5, the best scores not saturated
    images = []
    for target in (bound - 3, bound + 3):
        boxes, pred = _random_image(P, g, scale=1.0)
        scale, _ = _scale_for_count(pred, target)
        pred[:, : K + 1] *= scale
        images.append((boxes, pred, (200, 300)))
    sc = _scene(images)
    c0, c1 = _oracle_candidates(sc, 0), _oracle_candidates(sc, 1)
    assert bound - 5 <= c0 <= bound < c1 <= bound + 5, (c0, c1)
    ref = _oracle_det(sc)
    assert all(_well_posed(r) and len(r["scores"]) == TOPK for r in ref)
    out = _run_det_arms(sc, 0.9)
    assert int(out["err"]) == 0
    for i in range(2):
        _check_image(out, i, ref[i], 0.9)


# ---- A3: counts
def _five_proposals():
    """two suppressed pairs and a loner: 3 survivors (classes mixed so that the pairs are same-class)"""
    boxes = torch.tensor([[0.0, 0, 10, 10], [1.0, 0, 11, 10], [30.0, 0, 40, 10], [31.0, 0, 41, 10], [60.0, 0, 70, 10]])
    return boxes, _single_rows([1, 1, 4, 4, 0], [4.0, 3.5, 3.0, 2.5, 2.0]), (20, 80)


def test_det_no_proposals_and_no_candidates():
    """(a) pcount = [0, 37]; (b) an image whose foreground probabilities are all <= 0.05 (background logit 10): c == 0 in the sort, no
    chunk in the scan, dcount = pl_count = 0, every detection row zero with class -1"""
    g = torch.Generator().manual_seed(307)
    rb, rp = _random_image(37, g, scale=3.0)                    # (few candidates per row: fewer than topk detections)
    empty = (torch.zeros(0, 4), torch.zeros(0, CP), (200, 300))
    sc = _scene([empty, (rb, rp, (200, 300))])
    assert sc["pcount"] == [0, 37]
    ref = _oracle_det(sc)
    assert len(ref[0]["scores"]) == 0 and 0 < len(ref[1]["scores"]) < TOPK and _well_posed(ref[1])
    out = _run_det_arms(sc, 0.5)
    assert int(out["err"]) == 0
    for i in range(2):
        _check_image(out, i, ref[i], 0.5)
    assert int(out["dcount"][0]) == 0 and int(out["pl_count"][0]) == 0
    # (b)
    bb, bp = _random_image(300, g, scale=1.0)
    bp[:, K] = 10.0
    rb2, rp2 = _random_image(640, g)
    sc = _scene([(bb, bp, (200, 300)), (rb2, rp2, (190, 280))])
    assert _oracle_candidates(sc, 0) == 0 and float(torch.softmax(bp[:, : K + 1], -1)[:, :K].max()) <= 0.05
    ref = _oracle_det(sc)
    assert len(ref[0]["scores"]) == 0 and len(ref[1]["scores"]) == TOPK and _well_posed(ref[1])
    out = _run_det_arms(sc, 0.5)
    assert int(out["err"]) == 0
    for i in range(2):
        _check_image(out, i, ref[i], 0.5)
    assert int(out["dcount"][0]) == 0 and int(out["pl_count"][0]) == 0
    assert bool((out["db"][0] == 0).all()) and bool((out["ds"][0] == 0).all()) and bool((out["dc"][0] == -1).all())


def test_det_few_survivors_and_pseudolabel_count_edges():
    """(c) 5 proposals -> 3 survivors, beside an image with topk survivors; (d) pl_thresh below every score: pl_count == dcount; (e) above
    every score: pl_count == 0; (f) pl_rows = topk + 28: the whole tail -- boxes 0, scores 0, class -1 for np <= j < topk and 0 for j >= topk
    -- written over the sentinel"""
    g = torch.Generator().manual_seed(9)
    rb, rp = _random_image(640, g)
    sc = _scene([_five_proposals(), (rb, rp, (200, 300))])
    ref = _oracle_det(sc)
    assert len(ref[0]["scores"]) == 3 and ref[0]["pred_classes"].tolist() == [1, 4, 0]
    assert len(ref[1]["scores"]) == TOPK and _well_posed(ref[0]) and _well_posed(ref[1])
    lowest = min(float(r["scores"].min()) for r in ref)
    for thr, rows in ((0.9, TOPK), (0.9, TOPK + 28), (0.5 * lowest, TOPK), (0.5 * lowest, TOPK + 28), (1.0, TOPK), (1.0, TOPK + 28)):
        out = _run_det_arms(sc, thr, pl_rows=rows)
        assert int(out["err"]) == 0
        assert out["pb"].shape[1] == rows
        for i in range(2):
            k, m = _check_image(out, i, ref[i], thr)
            if thr < lowest:
                assert m == k > 0                                               # (d)
            if thr == 1.0:
                assert m == 0                                                   # (e)
        for key in ("pb", "pc", "ps"):                                          # (f) nothing of the sentinel is left
            assert not bool((out[key] == SENTINEL).any()), (thr, rows, key)
    assert int(out["dcount"][0]) == 3 and int(out["dcount"][1]) == TOPK


# ---- A4: strict comparisons
def test_det_iou_equal_to_threshold_and_identical_boxes_of_two_classes():
    """IoU exactly 0.5 (inter 8, union 16) does not suppress (`>`); an identical box of the same class is suppressed, the identical box of
    another class with the same score survives"""
    boxes = torch.tensor([[0.0, 0, 4, 4], [0.0, 0, 4, 2], [0.0, 0, 4, 4], [0.0, 0, 4, 4]])
    sc = _scene([(boxes, _single_rows([1, 1, 1, 5], [3.0, 2.0, 1.0, 1.0]), (10, 10)), _five_proposals()])
    ref = _oracle_det(sc)
    assert ref[0]["pred_classes"].tolist() == [1, 1, 5] and len(ref[1]["scores"]) == 3
    assert ref[0]["pred_boxes"].tolist() == [[0, 0, 4, 4], [0, 0, 4, 2], [0, 0, 4, 4]]
    out = _run_det_arms(sc, 0.8)
    assert int(out["err"]) == 0
    for i in range(2):
        _check_image(out, i, ref[i], 0.8)
    assert int(out["dcount"][0]) == 3 and int(out["pl_count"][0]) == 2


def test_det_score_equal_to_pl_thresh_is_no_pseudolabel():
    """a detection whose fp32 score is bit for bit the threshold is not a pseudo-label (strict `>`, as the reference's PseudoLabeler).  The
    threshold is the device's own det_scores[.., 1] of a first call; the expectation is the oracle's rule on the device's detections."""
    from oracle import aldi_ops as ao
    sc = _scene([_five_proposals(), _five_proposals()])
    first = _run_det_arms(sc, 0.5)
    assert first["dcount"].tolist() == [3, 3] and first["pl_count"].tolist() == [3, 3]
    thr = float(first["ds"][0, 1])
    assert torch.tensor(thr, dtype=torch.float32).item() == thr                  # passes through the C float argument unchanged
    out = _run_det_arms(sc, thr)
    for k in ("db", "ds", "dc", "dcount"):
        assert torch.equal(out[k], first[k])
    for n in range(2):
        k = int(out["dcount"][n])
        dev = {"image_size": sc["sizes"][n], "pred_boxes": out["db"][n, :k], "scores": out["ds"][n, :k], "pred_classes": out["dc"][n, :k].long()}
        pl = ao.process_bbox(dev, thr)
        assert len(pl["scores"]) == 1 and int(out["pl_count"][n]) == 1
        assert torch.equal(out["ps"][n, :1], pl["scores"]) and torch.equal(out["pb"][n, :1], pl["gt_boxes"])
        assert torch.equal(out["pc"][n, :1].long(), pl["gt_classes"])
        assert float(out["ds"][n, 1]) == thr and float(out["ps"][n, 0]) > thr


# ---- A5: the error word
def test_det_nonfinite_score_rows_are_dropped_and_flagged():
    """a row with a NaN logit and a row with a +inf logit: bit 2 of the error word, and every output as the oracle's, which drops those rows
    in inference"""
    g = torch.Generator().manual_seed(313)
    rb, rp = _random_image(640, g)
    rb2, rp2 = _random_image(300, g)
    clean = _oracle_det(_scene([(rb, rp, (200, 300)), (rb2, rp2, (190, 280))]))
    # the rows of image 0's two best candidates (both detections of the clean scene), so that dropping them shows
    best = torch.softmax(rp[:, : K + 1], -1)[:, :K].max(1)[0].argsort(descending=True)[:2].tolist()
    rp[best[0], 2] = float("nan")
    rp[best[1], 3] = float("inf")
    rp2[5, K] = float("nan")                                                     # (the background logit: no candidate of its own, the row still goes)
    sc = _scene([(rb, rp, (200, 300)), (rb2, rp2, (190, 280))])
    ref = _oracle_det(sc)
    assert all(_well_posed(r) for r in ref) and len(ref[0]["scores"]) == TOPK
    assert float(ref[0]["scores"][0]) < float(clean[0]["scores"][1])              # the oracle dropped both
    out = _run_det_arms(sc, 0.9)
    assert int(out["err"]) & 2
    assert int(out["err"]) & ~2 == 0
    for i in range(2):
        _check_image(out, i, ref[i], 0.9)


def test_det_more_candidates_than_capacity_is_flagged():
    """1100 rows of all-equal logits: 8800 candidates of probability 1/9 for 8192 slots.  Bit 4 of the error word, at most topk detections,
    everything finite (which candidates are dropped is unspecified; the writes are guarded by slot < capacity).  The other image of the batch
    is unaffected."""
    g = torch.Generator().manual_seed(17)
    boxes = _rand_boxes(1100, 300, 200, g, lo=8, hi=150)
    pred = torch.zeros(1100, CP)
    sc = _scene([(boxes, pred, (200, 300)), _five_proposals()])
    assert _oracle_candidates(sc, 0) == 8800
    ref1 = _oracle_det(_scene([_five_proposals()]))[0]
    for tri in (1, 0):
        out = _run_det(sc, 0.1, tri)
        assert int(out["err"]) & 4
        assert 0 < int(out["dcount"][0]) <= TOPK and 0 <= int(out["pl_count"][0]) <= int(out["dcount"][0])
        for k, v in out.items():
            assert bool(torch.isfinite(v.float()).all()), k
        _check_image(out, 1, ref1, 0.1)


# ------------------------------------------------------------------------------------------------
# RPN path
# ------------------------------------------------------------------------------------------------
A, C = 3, 16
SHAPES = [(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)]
RPN_ARMS = [(1, 1), (0, 1), (1, 0), (0, 0)]                                      # (rpn_topk_fused, nms_mask_tri)


def _rand_heads(shapes, N, g):
    heads = []
    for (h, w) in shapes:
        t = torch.randn(N, h, w, C, generator=g)
        t[..., A:] *= 0.5
        heads.append(t)
    return heads


def _oracle_rpn(shapes, heads, sizes, training):
    from oracle import d2_rcnn as d2
    cfg = _cfg()
    N = heads[0].shape[0]
    lo = [t[..., :A].reshape(N, -1) for t in heads]
    de = [t[..., A:5 * A].reshape(N, -1, 4) for t in heads]
    return d2.find_top_rpn_proposals(cfg, d2.generate_anchors(cfg, shapes), lo, de, sizes, training)


def _run_rpn(shapes, heads, sizes, training, fused, tri):
    from aldi_amd import _lib as L
    from aldi_amd import ops
    from aldi_amd.engine import make_anchors
    L.reset_tuning()
    L.set_tuning("rpn_topk_fused", fused)
    L.set_tuning("nms_mask_tri", tri)
    N = heads[0].shape[0]
    pre, post = (2000, 1000) if training else (1000, 1000)
    hd = [t.to(DEV) for t in heads]
    ws = torch.empty(ops.rpn_proposals_workspace(N, len(shapes)), dtype=torch.uint8, device=DEV)
    out = dict(boxes=torch.full((N, post, 4), SENTINEL, device=DEV), scores=torch.full((N, post), SENTINEL, device=DEV),
               count=torch.full((N,), int(SENTINEL), dtype=torch.int32, device=DEV), err=torch.zeros(1, dtype=torch.int32, device=DEV))
    ops.rpn_proposals(ops.make_geom(shapes, A, C), hd, make_anchors(shapes, DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV), N, pre, post, 0.7,
                      ws, out["boxes"], out["scores"], out["count"], out["err"])
    torch.cuda.synchronize()
    L.reset_tuning()
    return {k: v.cpu() for k, v in out.items()}


def _check_rpn(shapes, heads, sizes, training, ref, err_bits=0):
    """all four arms bit-identical; then scores bit-exact, boxes within 1e-3, exact count against the oracle; rows beyond the count zero"""
    outs = [_run_rpn(shapes, heads, sizes, training, f, t) for f, t in RPN_ARMS]
    for arm, o in zip(RPN_ARMS[1:], outs[1:]):
        for k in o:
            assert torch.equal(o[k], outs[0][k]), ("(rpn_topk_fused, nms_mask_tri)", arm, k)
    out = outs[0]
    assert int(out["err"]) == err_bits
    counts = []
    for n in range(len(sizes)):
        k = int(out["count"][n])
        assert k == len(ref[n]["proposal_boxes"]), (n, k, len(ref[n]["proposal_boxes"]))
        assert torch.equal(out["scores"][n, :k], ref[n]["objectness_logits"]), n
        if k:
            assert float((out["boxes"][n, :k] - ref[n]["proposal_boxes"]).abs().max()) < 1e-3, n
        assert bool((out["boxes"][n, k:] == 0).all()) and bool((out["scores"][n, k:] == 0).all()), n
        counts.append(k)
    return counts


def test_rpn_raster_chain():
    """32 x 32 anchors at stride 4 with zero deltas, scored in raster order: neighbours overlap at 0.78 > 0.7, second neighbours at 0.6 --
    a successor chain along every row of the map with vertical coupling between the rows, through all 32 chunks of the <2,16> scan
    instance.  Everything else ties at -20 (selection and merge by index and level)."""
    from oracle import d2_rcnn as d2
    shapes = [(16, 80), (8, 40), (4, 20), (2, 10), (1, 5)]
    an = d2.generate_anchors(_cfg(), shapes)[0]
    assert (an[1, 2] - an[1, 0]).item() == 32.0 and (an[1, 3] - an[1, 1]).item() == 32.0     # anchor 1 of a cell is the square one
    heads = [torch.zeros(2, h, w, C) for h, w in shapes]
    for t in heads:
        t[..., :A] = -20.0
    H, W = shapes[0]
    heads[0][0, :, :, 1] = torch.linspace(5.0, -5.0, H * W).view(H, W)
    heads[0][1, :, :, 1] = torch.linspace(5.0, -5.0, H * W).view(H, W).flip(1)                # image 1: the chain runs right to left
    sizes = [(64, 320), (64, 320)]
    for training in (True, False):
        ref = _oracle_rpn(shapes, heads, sizes, training)
        # 2000 candidates per level leave more than post_nms_topk survivors (the scans stop at 1000, the merge cuts); 1000 leave 787
        assert len(ref[0]["proposal_boxes"]) == (1000 if training else 787)
        counts = _check_rpn(shapes, heads, sizes, training, ref)
        assert counts[1] == 1000 if training else 0 < counts[1] < 1000


def test_rpn_total_tie_level():
    """every logit of the 9216-anchor level equal (more than pre_nms_topk: the k-th key's bucket holds the whole level, selection is the
    oracle's stable index order), random deltas; the small levels keep all their anchors (fewer than pre_nms_topk)"""
    g = torch.Generator().manual_seed(21)
    heads = _rand_heads(SHAPES, 2, g)
    heads[0][0, :, :, :A] = 0.5
    heads[0][1, :, :, :A] = -1.25
    heads[1][1, :, :, :A] = 0.25                                                  # 2304 anchors: tied too, above pre_nms_topk in both modes
    sizes = [(180, 250), (192, 256)]
    for training in (True, False):
        ref = _oracle_rpn(SHAPES, heads, sizes, training)
        counts = _check_rpn(SHAPES, heads, sizes, training, ref)
        assert min(counts) > 100


def test_rpn_emptied_image():
    """image 0: dx = 50 moves every box out of the image, clipping empties it, count 0 (the oracle's too); image 1 random and unaffected.
    Then images far smaller than the feature map: most anchors clip to empty."""
    g = torch.Generator().manual_seed(23)
    heads = _rand_heads(SHAPES, 2, g)
    for t in heads:
        t[0, :, :, A:5 * A:4] = 50.0
    sizes = [(180, 250), (192, 256)]
    for training in (True, False):
        ref = _oracle_rpn(SHAPES, heads, sizes, training)
        assert len(ref[0]["proposal_boxes"]) == 0 and len(ref[1]["proposal_boxes"]) > 100
        assert _check_rpn(SHAPES, heads, sizes, training, ref)[0] == 0
    heads = _rand_heads(SHAPES, 2, g)
    sizes = [(20, 30), (40, 24)]
    for training in (True, False):
        ref = _oracle_rpn(SHAPES, heads, sizes, training)
        counts = _check_rpn(SHAPES, heads, sizes, training, ref)
        assert all(0 < c < 1000 for c in counts)


def test_rpn_nonfinite_logits_in_inference():
    """NaN and +inf logits (they sort first and take a slot of the pre-NMS top-k, in the oracle's torch.sort as in the device's keys) and a
    -inf logit on a level that keeps all its anchors: bit 1 of the error word -- the engine raises FloatingPointError on it in training and
    inference alike (engine.raise_on_error) -- and the proposals are the oracle's, which drops those boxes in inference."""
    g = torch.Generator().manual_seed(27)
    heads = _rand_heads(SHAPES, 2, g)
    heads[0][0, 7, 9, 1] = float("nan")
    heads[1][0, 3, 4, 2] = float("inf")
    heads[4][1, 1, 2, 0] = float("-inf")
    heads[0][1, 40, 60, 0] = float("inf")
    sizes = [(180, 250), (192, 256)]
    ref = _oracle_rpn(SHAPES, heads, sizes, False)
    assert all(bool(torch.isfinite(r["objectness_logits"]).all()) for r in ref)
    counts = _check_rpn(SHAPES, heads, sizes, False, ref, err_bits=1)
    assert min(counts) > 100

"""Operands and references for the exact tests of the training-side label pipeline (csrc/rpn.hip: aldi_box_match, aldi_compact_labels,
aldi_rpn_apply_sample, aldi_roi_prepare_lists; csrc/roi.hip: aldi_roi_gather).  CPU only: test_label_pipeline_cpu.py pins what is here
without a GPU, test_label_pipeline_gpu.py compares every arm of every kernel with it.  Every comparison is bit equality.

The matcher's operands are LATTICE boxes: non-negative integer coordinates, small enough that every area, every intersection and every
union is an integer below 2^24 and the sum of two overlapping boxes' areas is exact in fp32 (`assert_lattice`).  Every fp32 operation of the IoU before the division is then
exact, and the IoU is the correctly rounded quotient of two exact integers -- the same bits on the device, in the fp32 oracle and in
the integer reference below (float32(float64(inter) / float64(union)): with 24-bit operands the detour through fp64 rounds the same).

Two references, which must agree on every scene: the project's oracle (oracle.d2_rcnn.pairwise_iou + matcher, fp32) and `int_match`
(integer areas, first maximum, [lo, hi) label intervals, low-quality rule `IoU == best of that GT over all boxes`)."""
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

LIM = 1 << 24
FILLER = (5000, 5000, 5010, 5010)          # overlaps no GT of any scene
WAVE = 64
BIG_L = 65573                              # past 65536, not a multiple of 64: the last wave has 37 active lanes
BIG_TAIL = BIG_L - (BIG_L // WAVE) * WAVE  # 37


# ------------------------------------------------------------------------------------------------
# integer IoU and the two matchers
# ------------------------------------------------------------------------------------------------
def assert_lattice(gt: torch.Tensor, boxes: torch.Tensor) -> None:
    """the precondition of bit equality: integers >= 0, every quantity of the IoU below 2^24"""
    for t in (gt, boxes):
        assert t.dtype == torch.int64 and (t.numel() == 0 or int(t.min()) >= 0)
        assert t.numel() == 0 or int(t.max()) < LIM
        assert bool((t[:, 2] >= t[:, 0]).all()) and bool((t[:, 3] >= t[:, 1]).all())
    if gt.numel() == 0 or boxes.numel() == 0:
        return
    inter, union = int_inter_union(gt, boxes)
    ov = inter > 0                                   # (a pair that does not overlap has IoU 0 whatever its areas are)
    asum = (int_area(gt)[:, None] + int_area(boxes)[None, :])[ov]
    assert bool((union[ov] < LIM).all()) and int(int_area(gt).max()) < LIM and int(int_area(boxes).max()) < LIM
    assert bool((asum.float().long() == asum).all())  # area1 + area2, formed before the intersection is subtracted, is exact in fp32


def int_area(b: torch.Tensor) -> torch.Tensor:
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def int_inter_union(gt: torch.Tensor, boxes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(G, M) int64 intersection and union"""
    w = (torch.minimum(gt[:, None, 2], boxes[None, :, 2]) - torch.maximum(gt[:, None, 0], boxes[None, :, 0])).clamp(min=0)
    h = (torch.minimum(gt[:, None, 3], boxes[None, :, 3]) - torch.maximum(gt[:, None, 1], boxes[None, :, 1])).clamp(min=0)
    inter = w * h
    return inter, int_area(gt)[:, None] + int_area(boxes)[None, :] - inter


def int_iou(gt: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """(G, M) fp32: inter > 0 ? correctly rounded inter / union : 0"""
    inter, union = int_inter_union(gt, boxes)
    q = (inter.double() / union.clamp(min=1).double()).float()
    return torch.where(inter > 0, q, torch.zeros((), dtype=torch.float32))


def int_match(gt: torch.Tensor, boxes: torch.Tensor, lo: float, hi: float, lowq: bool, *, last_max: bool = False, strict_ge: bool = False,
              lowq_needs_overlap: bool = False, iou: Optional[torch.Tensor] = None):
    """(best_iou fp32 [M], best_idx int64 [M], labels int64 [M]).  G == 0: IoU -1 (the kernels' "nothing seen"), index 0, label 0.
    The keyword flags are the deliberately WRONG variants the CPU test holds against the scenes:
      last_max            the last maximum wins instead of the first
      strict_ge           `>` for `>=` at both thresholds
      lowq_needs_overlap  the low-quality rule only for IoU > 0 (a GT nothing overlaps claims nobody)"""
    G, M = gt.shape[0], boxes.shape[0]
    if G == 0 or M == 0:
        return torch.full((M,), -1.0), torch.zeros(M, dtype=torch.int64), torch.zeros(M, dtype=torch.int64)
    iou = int_iou(gt, boxes) if iou is None else iou
    best = iou.max(dim=0).values
    ar = torch.arange(G)[:, None].expand(G, M)
    at_max = iou == best[None, :]
    idx = torch.where(at_max, ar, torch.full_like(ar, -1)).max(dim=0).values if last_max else torch.where(at_max, ar, torch.full_like(ar, G)).min(dim=0).values
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    below_lo = best <= lo32 if strict_ge else best < lo32
    below_hi = best <= hi32 if strict_ge else best < hi32
    labels = torch.where(below_lo, 0, torch.where(below_hi, -1, 1)).to(torch.int64)
    if lowq:
        hit = iou == iou.max(dim=1).values[:, None]
        if lowq_needs_overlap:
            hit = hit & (iou > 0)
        labels = torch.where(hit.any(dim=0), torch.ones_like(labels), labels)
    return best, idx, labels


def oracle_match(gt: torch.Tensor, boxes: torch.Tensor, lo: float, hi: float, lowq: bool, mqm: Optional[torch.Tensor] = None):
    """the same through oracle.d2_rcnn in fp32 (lo == hi: the single-threshold matcher of the ROI heads)"""
    from oracle import d2_rcnn as d2
    M = boxes.shape[0]
    if gt.shape[0] == 0 or M == 0:
        return torch.full((M,), -1.0), torch.zeros(M, dtype=torch.int64), torch.zeros(M, dtype=torch.int64)
    mqm = d2.pairwise_iou(gt.float(), boxes.float()) if mqm is None else mqm
    if lo == hi:
        idx, lab = d2.matcher(mqm, [lo], [0, 1], lowq)
    else:
        idx, lab = d2.matcher(mqm, [lo, hi], [0, -1, 1], lowq)
    return mqm.max(dim=0).values, idx.to(torch.int64), lab.to(torch.int64)


# ------------------------------------------------------------------------------------------------
# the GT lists of the culling kernels, as a model: which GTs a wave (or a workgroup) walks
# ------------------------------------------------------------------------------------------------
def cull_lists(gt: torch.Tensor, boxes: torch.Tensor, count: int, L: int, group: int = WAVE, *, widen_inactive: bool = False) -> List[List[int]]:
    """per group of `group` consecutive box slots of an L-slot list: the ascending GT indices whose box meets the union box of the group's
    ACTIVE slots (index < count) with positive width and height.  widen_inactive is the WRONG variant in which inactive lanes enter the
    union with the [0, 0, 0, 0] they hold.  A wider union only lengthens a list (labels cannot change: IoU with an extra GT is 0 for
    every box of the group), so the variant shows in the lists and in nothing else -- it is the kernels' time that it costs."""
    out = []
    for s in range(0, L, group):
        act = boxes[s:min(s + group, count)]
        if widen_inactive and min(s + group, count) < s + group:
            act = torch.cat([act, torch.zeros(1, 4, dtype=boxes.dtype)])
        if act.shape[0] == 0:
            out.append([])
            continue
        x0, y0, x1, y1 = int(act[:, 0].min()), int(act[:, 1].min()), int(act[:, 2].max()), int(act[:, 3].max())
        out.append([g for g in range(gt.shape[0])
                    if min(int(gt[g, 2]), x1) - max(int(gt[g, 0]), x0) > 0 and min(int(gt[g, 3]), y1) - max(int(gt[g, 1]), y0) > 0])
    return out


def culled_match(gt: torch.Tensor, boxes: torch.Tensor, count: int, L: int, lo: float, hi: float, lowq: bool, group: int = WAVE):
    """int_match computed the kernels' way: every group of boxes sees only its culled list.  Equal to int_match when culling is sound."""
    M = count
    if gt.shape[0] == 0 or M == 0:
        return int_match(gt, boxes[:M], lo, hi, lowq)
    iou = int_iou(gt, boxes[:M])
    seen = torch.zeros_like(iou, dtype=torch.bool)
    for k, lst in enumerate(cull_lists(gt, boxes, count, L, group)):
        if lst:
            seen[torch.tensor(lst), k * group:min((k + 1) * group, M)] = True
    iou = torch.where(seen, iou, torch.zeros((), dtype=torch.float32))
    best, idx = torch.zeros(M), torch.zeros(M, dtype=torch.int64)
    for g in range(gt.shape[0]):                          # running maximum from (0, index 0), strictly greater to replace
        better = iou[g] > best
        best, idx = torch.where(better, iou[g], best), torch.where(better, torch.full_like(idx, g), idx)
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    labels = torch.where(best < lo32, 0, torch.where(best < hi32, -1, 1)).to(torch.int64)
    if lowq:
        top = iou.max(dim=1).values
        hit = ((iou == top[:, None]) & (iou > 0)).any(dim=0) | bool((top == 0).any())
        labels = torch.where(hit, torch.ones_like(labels), labels)
    return best, idx, labels


# ------------------------------------------------------------------------------------------------
# quotients next to a threshold
# ------------------------------------------------------------------------------------------------
def f32_of_fraction(p: int, u: int) -> np.float32:
    return np.float32(np.float64(p) / np.float64(u))


def nearest_quotients(num: int, den: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """the quotients p/u closest below and closest above num/den (in lowest terms) that two lattice boxes can have as (intersection,
    union): a box of p unit cells nested in a GT of u cells has IoU p/u, for every 0 < p < u with p + u < 2^24 (the sum of the two areas is
    formed in fp32 before the intersection is subtracted).  |num/den - p/u| = r / (den u) with the integer r = |num u - den p| >= 1, and
    r = 1 occurs once in every den consecutive u, so the closest quotient has u within den of the largest admissible u: the search over
    the last 8192 values of u is exhaustive."""
    ub = LIM * den // (num + den)                         # p + u < 2^24 with p ~ u num / den
    u = np.arange(max(2, ub - 8192), min(LIM, ub + 64), dtype=np.int64)
    best = []
    for below in (True, False):
        p = (num * u - 1) // den if below else (num * u) // den + 1          # largest p with p/u < num/den, smallest with p/u > num/den
        ok = (p > 0) & (p < u) & (p + u < LIM)
        cands = [(int(a), int(b)) for a, b in zip(p[ok], u[ok])]
        best.append(min(cands, key=lambda c: abs(Fraction(num, den) - Fraction(c[0], c[1]))))
    return best[0], best[1]


THRESHOLDS = ((3, 10, 0.3), (7, 10, 0.7), (1, 2, 0.5))
# which side of float32(threshold) the correctly rounded neighbours fall on, as found by nearest_quotients and worked out by hand:
# the neighbours are 1/(den * u) away with u ~ 1e7, a fraction of the ulp (3e-8 below 0.5, 6e-8 above), so the one on the side where
# float32(threshold) itself lies (0.3f = 3/10 + 1.2e-8, above) rounds ONTO the threshold; 0.7f = 7/10 - 1.2e-8 is closer to BOTH neighbours
# of 7/10 (1e-8 away from it) than the next fp32 value 6e-8 further; 1/2 is exact and its neighbours are 4.5e-8 away, past half an ulp.
#   name -> (below: "lt" | "eq" | "gt" relative to float32(thr), above: ...)
NEIGHBOUR_SIDES = {"3/10": ("lt", "eq"), "7/10": ("eq", "eq"), "1/2": ("lt", "gt")}


def side(p: int, u: int, thr: float) -> str:
    q, t = f32_of_fraction(p, u), np.float32(thr)
    return "lt" if q < t else ("eq" if q == t else "gt")


# ------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------
@dataclass
class Scene:
    """groups: per image, a list of box groups.  A group occupies one 64-aligned wave of the box list: it is padded to 64 with copies of
    its first box (so that a wave's union box is the union of the group), except the LAST group, which is ragged (<= 37 boxes: the last
    wave of the big layout has 37 lanes).  gt: per image the GT boxes (rows past the image's count are copies of GT 0, to be ignored)."""
    name: str
    groups: List[List[List[Tuple[int, int, int, int]]]]
    gt: List[List[Tuple[int, int, int, int]]]
    gmax: int
    configs: Sequence[Tuple[float, float, bool]]
    count_of: Optional[List[Callable[[int], int]]] = None        # box_count per image as a function of L (None: no box_count argument)
    stride_pad: int = 0                                          # box_stride_n = L + stride_pad
    facts: dict = field(default_factory=dict)                    # the edge each scene carries, checked by the CPU test

    @property
    def N(self):
        return len(self.groups)


RPN_CFG = ((0.3, 0.7, True), (0.3, 0.7, False))
ALL_CFG = RPN_CFG + ((0.5, 0.5, False),)


def layout(scene: Scene, big: bool):
    """(boxes int64 [N, L, 4], L, positions): the scene's groups in a box list.  small: the groups back to back.  big: L = 65573, the
    first group at the start, the second and third across the 1023 / 1024 boundary (waves 15 and 16: two workgroups of the 1024-thread
    kernels), further ones behind, the last in the ragged last wave; FILLER everywhere else."""
    ng = max(len(g) for g in scene.groups)
    assert all(len(g) == ng for g in scene.groups)
    if big:
        L = BIG_L
        pos = [0, 15 * WAVE, 16 * WAVE] + [(32 + 7 * k) * WAVE for k in range(ng)]
        pos = pos[:ng - 1] + [(BIG_L // WAVE) * WAVE]
    else:
        last = max(len(g[-1]) for g in scene.groups)
        L = (ng - 1) * WAVE + last
        pos = [k * WAVE for k in range(ng)]
    boxes = torch.tensor(FILLER, dtype=torch.int64).repeat(scene.N, L, 1)
    for n, groups in enumerate(scene.groups):
        for k, grp in enumerate(groups):
            assert 0 < len(grp) <= (BIG_TAIL if k == ng - 1 else WAVE)
            g = torch.tensor(grp, dtype=torch.int64)
            if k < ng - 1:
                g = torch.cat([g, g[:1].repeat(WAVE - len(grp), 1)])
            boxes[n, pos[k]:pos[k] + g.shape[0]] = g
    return boxes, L, pos


def gt_tensor(scene: Scene):
    """(gt int64 [N, Gmax, 4], counts list)"""
    out = torch.zeros(scene.N, scene.gmax, 4, dtype=torch.int64)
    counts = []
    for n, g in enumerate(scene.gt):
        counts.append(len(g))
        assert len(g) <= scene.gmax
        if g:
            out[n, :len(g)] = torch.tensor(g, dtype=torch.int64)
            out[n, len(g):] = out[n, 0]                   # rows past the count: a GT that WOULD match if read
    return out, counts


def box_counts(scene: Scene, L: int) -> List[int]:
    return [L] * scene.N if scene.count_of is None else [f(L) for f in scene.count_of]


def chunk(boxes: List[Tuple[int, int, int, int]], last: int) -> List[List[Tuple[int, int, int, int]]]:
    """a flat box list as groups: the final `last` boxes are the ragged group, the others full groups of 64"""
    head, tail = boxes[:-last], boxes[-last:]
    return [head[i:i + WAVE] for i in range(0, len(head), WAVE)] + [tail]


def strip(p: int, u: int, y: int):
    """(box, gt) with IoU exactly p/u: p unit cells nested in u unit cells, on row y"""
    return (0, y, p, y + 1), (0, y, u, y + 1)


def scene_threshold() -> Scene:
    """IoUs exactly 3/10, 7/10, 1/2 and the closest lattice quotients on either side of each.  Every GT also has a champion (a box equal
    to it, IoU 1, in another wave), so that the low-quality rule does not lift the boxes under test to 1."""
    tested, champs, gts, names = [], [], [], []
    y = 0
    for num, den, thr in THRESHOLDS:
        below, above = nearest_quotients(num, den)
        for tag, (p, u) in (("exact", (num, den)), ("below", below), ("above", above)):
            b, g = strip(p, u, y)
            tested.append(b); gts.append(g); champs.append(g); names.append((f"{num}/{den}", tag, p, u, thr))
            y += 2
    # a second exact pair per threshold that is not nested: box [0, a) and GT [a - o, a - o + b) on one row, o / (a + b - o)
    for (a, o, bb) in ((6, 3, 7), (8, 7, 9), (2, 1, 1)):
        tested.append((0, y, a, y + 3)); gts.append((a - o, y, a - o + bb, y + 3)); champs.append(gts[-1])
        y += 4
    return Scene("threshold", [[tested, champs[:BIG_TAIL]]], [gts], 16, ALL_CFG, facts=dict(pairs=names))


def _cover(k):
    return (0, 0, 60, 30 + k)                    # distinct GTs that cover every box of the ties scene with a small IoU


def scene_ties() -> Scene:
    """a duplicated GT and two different GTs with one IoU (100/150): the lower index wins.  16 GTs that all meet every workgroup's
    union, so the four quarters of the parts == 4 kernel hold indices 0-3, 4-7, 8-11, 12-15.
    image 0: the duplicates at 1 and 2, the equal pair at 5 and 6 (each within one quarter); image 1: 1 and 14, 2 and 9 (across quarters)"""
    b0, b1 = (10, 10, 20, 20), (40, 10, 50, 20)
    dup, eq_a, eq_b = (10, 10, 20, 25), (40, 10, 50, 25), (35, 10, 50, 20)
    imgs, where = [], []
    for (d0, d1, e0, e1) in ((1, 2, 5, 6), (1, 14, 2, 9)):
        g = [_cover(k) for k in range(16)]
        g[d0] = g[d1] = dup
        g[e0], g[e1] = eq_a, eq_b
        imgs.append(g); where.append(dict(dup=(d0, d1), eq=(e0, e1)))
    groups = [[[b0, b1, (0, 0, 5, 5)], [b1, b0]] for _ in imgs]
    return Scene("ties", groups, imgs, 16, ALL_CFG, facts=dict(where=where, box_dup=0, box_eq=1))


def scene_low_quality() -> Scene:
    """image 0 (G = 1): a GT whose best IoU is 1/10 < lo, reached by three boxes: all three get label 1 with the rule, 0 without
    image 1 (G = Gmax): the same plus ordinary GTs and a GT nothing overlaps, which claims EVERY box
    image 2 (G = 0): label 0, index 0
    image 3 (G = 3): a zero-area GT inside a box (IoU 0 with everything): claims every box as well
    image 4 (G = Gmax): ordinary GTs only -- the rule lifts exactly the per-GT best boxes"""
    tall = (0, 0, 10, 100)
    boxes = [(0, 0, 10, 10), (0, 10, 10, 20), (0, 20, 10, 30), (200, 0, 220, 20), (200, 0, 220, 30), (300, 0, 310, 10), (400, 400, 410, 410)]
    ordinary = [(200, 0, 220, 24), (300, 0, 312, 12), (296, 0, 310, 10), (204, 2, 216, 20)]
    gt = [[tall], [tall] + ordinary[:3] + [(9000, 9000, 9010, 9010)], [], [tall, ordinary[0], (205, 5, 205, 9)], [tall] + ordinary]
    groups = [[boxes[:4], boxes[4:]] for _ in gt]
    return Scene("low_quality", groups, gt, 5, RPN_CFG, facts=dict(three=(0, 1, 2), claims_all=(1, 3), no_gt=2))


def scene_culling() -> Scene:
    """wave-level culling.  group 0: two boxes 90 apart; GT 0 lies in the gap (meets the union, no box), GT 1 shares only the edge
    x = 210 with the union.  group 1: 32 + 32 boxes from two clusters 2000 apart, GT 4 / GT 5 overlap one cluster each, GT 6 lies between.
    group 2: the champions (boxes equal to GTs 0, 1, 3, 6, so that no GT has a zero best and the low-quality rule stays selective).
    last group (ragged: lanes past it are inactive and hold [0, 0, 0, 0]): every box far from the origin, GT 3 AT the origin; GT 2
    overlaps only the LAST active box."""
    gt = [(140, 102, 160, 108), (210, 100, 230, 110), (302, 302, 312, 312), (0, 0, 5, 5),
          (1000, 1000, 1012, 1012), (3004, 3004, 3014, 3014), (2000, 2000, 2010, 2010)]
    g0 = [(100, 100, 110, 110), (200, 100, 210, 110)]
    g1 = [(1000 + i, 1000, 1010 + i, 1010) for i in range(32)] + [(3000, 3000 + i, 3010, 3010 + i) for i in range(32)]
    g2 = [gt[0], gt[1], gt[3], gt[6]]
    tail = [(100, 300, 110, 310)] * (BIG_TAIL - 1) + [(300, 300, 310, 310)]
    return Scene("culling", [[g0, g1, g2, tail]], [gt], 8, ALL_CFG, facts=dict(gap=(0, 0), edge=(0, 1), clusters=(1, 6), origin=3, last_only=2))


def _grid_gt(k):
    return (20 * (k % 20), 20 * (k // 20), 20 * (k % 20) + 12, 20 * (k // 20) + 12)


def scene_tiles() -> Scene:
    """Gmax = 300, G = 257 and 300: a 20 x 15 grid of disjoint 12 x 12 GTs, a champion box on each, and boxes whose best GT is in the
    second 256-tile (256, 259, 299), on the boundary (255 | 256: a box covering both equally -- 255 wins) and in the first.  Image 1
    has GT 259 = GT 3 (a duplicate across the tiles: 3 wins).  In image 0 (G = 257) the boxes at GTs 257 .. 299 overlap nothing."""
    def shifted(k):
        x0, y0, x1, y1 = _grid_gt(k)
        return (x0 + 2, y0, x1 + 2, y1)
    special = [shifted(k) for k in (0, 3, 100, 255, 256, 259, 299)] + [(_grid_gt(255)[0], _grid_gt(255)[1], _grid_gt(256)[2], _grid_gt(256)[3])]
    champs = [_grid_gt(k) for k in range(300)]
    g0 = [_grid_gt(k) for k in range(257)]
    g1 = [_grid_gt(k) for k in range(300)]
    g1[259] = g1[3]
    groups = chunk(champs + special, 20)
    return Scene("tiles", [groups, groups], [g0, g1], 300, ALL_CFG)


def scene_counts() -> Scene:
    """box_count below L (one image at 0), box_stride_n != L.  Slots past the count hold a copy of GT 0 -- reading one shows"""
    g = torch.Generator().manual_seed(11)

    def rnd(n):
        xy = torch.randint(0, 160, (n, 2), generator=g)
        wh = torch.randint(4, 60, (n, 2), generator=g)
        return [tuple(int(v) for v in r) for r in torch.cat([xy, xy + wh], 1)]
    gts = [rnd(3), rnd(2), rnd(4)]
    groups = []
    for n in range(3):
        flat = rnd(64 + 64 + 30)
        flat[5] = gts[n][1]                                  # a box equal to a GT
        groups.append([flat[:64], flat[64:128], flat[128:]])
    return Scene("counts", groups, gts, 4, ALL_CFG, count_of=[lambda L: L - 5, lambda L: 0, lambda L: 70], stride_pad=3)


SCENES = {f.__name__[6:]: f for f in (scene_threshold, scene_ties, scene_low_quality, scene_culling, scene_tiles, scene_counts)}
_scene_cache = {}


def scene(name: str) -> Scene:
    if name not in _scene_cache:
        _scene_cache[name] = SCENES[name]()
    return _scene_cache[name]


_ref_cache = {}
_iou_cache = {}


def operands(sc: Scene, big: bool):
    """what the device call takes: boxes int64 [N, L + stride_pad, 4] with every slot past an image's box_count (and the stride padding)
    holding a copy of the image's GT 0 (a box that WOULD match if it were read), L, the box counts (None: no box_count argument),
    gt int64 [N, Gmax, 4], the GT counts"""
    boxes, L, _ = layout(sc, big)
    gt, gcnt = gt_tensor(sc)
    out = torch.zeros(sc.N, L + sc.stride_pad, 4, dtype=torch.int64)
    out[:, :L] = boxes
    for n, cnt in enumerate(box_counts(sc, L)):
        out[n, cnt:] = gt[n, 0]
    return out, L, (None if sc.count_of is None else box_counts(sc, L)), gt, gcnt


def references(name: str, big: bool, cfg: Tuple[float, float, bool]):
    """per image (best_iou, best_idx, labels) over the image's ACTIVE boxes, from both references: (int_refs, oracle_refs); computed once"""
    key = (name, big, cfg)
    if key not in _ref_cache:
        sc = scene(name)
        boxes, L, _ = layout(sc, big)
        gt, gcnt = gt_tensor(sc)
        from oracle import d2_rcnn as d2
        ints, orcs = [], []
        for n, cnt in enumerate(box_counts(sc, L)):
            # IoU, first maximum, label and the per-GT best over all boxes depend on the SET of distinct boxes only: match those (the big
            # layout is 65 k copies of one filler box around the scene) and give every slot its box's result
            g = gt[n, :gcnt[n]]
            if (name, big, n) not in _iou_cache:
                b, inv = torch.unique(boxes[n, :cnt], dim=0, return_inverse=True)
                assert_lattice(g, b)
                _iou_cache[(name, big, n)] = (b, inv) + ((int_iou(g, b), d2.pairwise_iou(g.float(), b.float())) if g.shape[0] and cnt else (None, None))
            b, inv, iou, mqm = _iou_cache[(name, big, n)]
            ints.append(tuple(x[inv] for x in int_match(g, b, *cfg, iou=iou)))
            orcs.append(tuple(x[inv] for x in oracle_match(g, b, *cfg, mqm=mqm)))
        _ref_cache[key] = (ints, orcs)
    return _ref_cache[key]


# ------------------------------------------------------------------------------------------------
# the dispatch of aldi_box_match, read from csrc/rpn.hip
# ------------------------------------------------------------------------------------------------
ARMS = {
    # name: (big list, padded scratch, match_wave knob or None where it is not read)
    "wg256_parts4": (False, False, None),     # small list, Gmax <= 256: match_iou_kernel, 256 threads, four waves share the GT list
    "wg64": (False, False, None),             # small list, Gmax > 256: match_iou_kernel, one wave per workgroup, 64-entry tiles
    "wg1024": (True, False, 0),               # big list, match_wave 0: match_iou_kernel, 1024 threads, one list per workgroup
    "wave_packed": (True, False, 1),          # big list, match_wave 1: match_iou_wave_kernel / match_label_wave_kernel, packed scratch
    "wave_padded_small": (False, True, None),  # ops.box_match_scratch (a 128-byte line per GT) selects the wave kernels at any size
    "wave_padded_big": (True, True, None),
}


def select_arm(L: int, N: int, Gmax: int, scratch_bytes: int, match_wave: int) -> str:
    """the arm aldi_box_match takes"""
    assert scratch_bytes >= 4 * N * Gmax
    padded = scratch_bytes >= N * Gmax * 128
    big = L * N >= (1 << 16)
    if padded:
        return "wave_padded_big" if big else "wave_padded_small"
    if big:
        return "wave_packed" if match_wave != 0 else "wg1024"
    return "wg256_parts4" if Gmax <= 256 else "wg64"


def arms_for(sc: Scene) -> List[str]:
    return [a for a in ARMS if not (a == "wg256_parts4" and sc.gmax > 256) and not (a == "wg64" and sc.gmax <= 256)]


# ------------------------------------------------------------------------------------------------
# B: label lists, sampling, ROI preparation, ROI gather
# ------------------------------------------------------------------------------------------------
COMPACT_L = (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 65 * 4096 + 1)
LABEL_PATTERNS = ("all_pos", "all_bg", "all_ignore", "all_pad", "alternating", "first_only", "last_only", "segment_firsts")


def label_pattern(kind: str, L: int, bg: int, K: int) -> torch.Tensor:
    """int32 [L] labels; positives are 1 for bg == 0 and cycle through the classes 0 .. K - 1 for bg == K"""
    i = torch.arange(L)
    pos = torch.ones(L, dtype=torch.int64) if bg == 0 else i % K
    bgv = torch.full((L,), bg)
    if kind == "all_pos":
        v = pos
    elif kind == "all_bg":
        v = bgv
    elif kind == "all_ignore":
        v = torch.full((L,), -1)
    elif kind == "all_pad":
        v = torch.full((L,), -2)
    elif kind == "alternating":
        v = torch.where(i % 2 == 0, pos, bgv)
    elif kind == "first_only":
        v = torch.where(i == 0, pos, torch.full((L,), -1))
    elif kind == "last_only":
        v = torch.where(i == L - 1, bgv, torch.full((L,), -2))
    elif kind == "segment_firsts":
        v = torch.where(i % 4096 == 0, torch.where((i // 4096) % 2 == 0, pos, bgv), torch.full((L,), -1))
    else:
        raise KeyError(kind)
    return v.to(torch.int32)


def compact_ref(labels: torch.Tensor, bg: int):
    """subsample_labels' two index lists: (positive, negative) int64, ascending (torch.nonzero)"""
    pos = torch.nonzero((labels != -1) & (labels != -2) & (labels != bg)).squeeze(1)
    neg = torch.nonzero(labels == bg).squeeze(1)
    return pos, neg


def roi_scene(P: int, Gmax: int, seed: int = 3):
    """four images of lattice proposals and GTs for aldi_roi_prepare_lists:
    image 0: proposal 0 equal to GT 0, proposal 1 with IoU exactly 1/2 (foreground at 0.5), proposal 2 with 2/5, GT 1 a copy of GT 0
             (where Gmax > 1), gt_count = Gmax, pcount = P - 2
    image 1: pcount = 0 with GTs present; image 2: gt_count = 0 (all background, class K); image 3: both zero"""
    g = torch.Generator().manual_seed(seed + P + Gmax)

    def rnd(n):
        xy = torch.randint(0, 300, (n, 2), generator=g)
        wh = torch.randint(4, 80, (n, 2), generator=g)
        return torch.cat([xy, xy + wh], 1)
    N, K = 4, 8
    props, gt = torch.zeros(N, P, 4, dtype=torch.int64), torch.zeros(N, Gmax, 4, dtype=torch.int64)
    for n in range(N):
        props[n], gt[n] = rnd(P), rnd(Gmax)
    gt[0, 0] = torch.tensor([10, 10, 20, 20])
    if Gmax > 1:
        gt[0, 1] = gt[0, 0]
    props[0, 0] = gt[0, 0]
    props[0, 1] = torch.tensor([10, 10, 20, 15])
    props[0, 2] = torch.tensor([10, 10, 20, 14])
    gcls = torch.randint(0, K, (N, Gmax), generator=g)
    if Gmax > 1:
        gcls[0, 1] = (gcls[0, 0] + 1) % K                       # the duplicate has ANOTHER class: the lower index must give the class
    pcount = [P - 2, 0, P, 0]
    gcount = [Gmax, max(1, Gmax // 2), 0, 0]
    return dict(N=N, K=K, P=P, Gmax=Gmax, props=props, gt=gt, gcls=gcls, pcount=pcount, gcount=gcount)


def roi_prepare_ref(sc: dict, thr: float = 0.5):
    """oracle.d2_rcnn.label_and_sample_proposals up to its random draw, per image: its own statements (add the GT to the proposals,
    pairwise_iou, matcher([thr], [0, 1], no low-quality rule), classes with background K), then the two lists subsample_labels draws from"""
    from oracle import d2_rcnn as d2
    out = []
    for n in range(sc["N"]):
        pc, gc, K = sc["pcount"][n], sc["gcount"][n], sc["K"]
        gtb, gtc = sc["gt"][n, :gc].float(), sc["gcls"][n, :gc].to(torch.int64)
        pb = sc["props"][n, :pc].float()
        if gc > 0:
            pb = torch.cat([pb, gtb])
        mqm = d2.pairwise_iou(gtb, pb)
        midx, mlab = d2.matcher(mqm, [thr], [0, 1], False)
        if gc > 0:
            cls = gtc[midx]
            cls[mlab == 0] = K
            best = mqm.max(dim=0).values
        else:
            cls = torch.zeros_like(midx) + K
            best = torch.full((pb.shape[0],), -1.0)
        fg = torch.nonzero((cls != -1) & (cls != K)).squeeze(1)
        bg = torch.nonzero(cls == K).squeeze(1)
        out.append(dict(cand=pb, count=pc + gc, midx=midx, lab=mlab.to(torch.int64), cls=cls, best=best, fg=fg, bg=bg))
    return out


def roi_gather_ref(cand, cls, best_idx, lists, sel, nsel, row_off, gt, gcount, R: int, sentinel: float):
    """sampled_idxs = cat(fg_list[sel_fg], bg_list[sel_bg]) per image, rows from row_off[n]; rows outside keep the sentinel.
    cand [N, L, 4] fp32, cls / best_idx [N, L], lists [N, 2, L], sel [N, 2, S], nsel [N, 2], gt [N, Gmax, 4] fp32"""
    rois = torch.full((R, 5), sentinel)
    r_cls = torch.full((R,), int(sentinel), dtype=torch.int64)
    r_gt = torch.full((R, 4), sentinel)
    r_idx = torch.full((R,), int(sentinel), dtype=torch.int64)
    for n in range(cand.shape[0]):
        nf, nb = int(nsel[n, 0]), int(nsel[n, 1])
        idx = torch.cat([lists[n, 0][sel[n, 0, :nf].long()], lists[n, 1][sel[n, 1, :nb].long()]]).long()
        rows = slice(int(row_off[n]), int(row_off[n]) + nf + nb)
        rois[rows, 0] = float(n)
        rois[rows, 1:] = cand[n][idx]
        r_cls[rows] = cls[n][idx].long()
        r_gt[rows] = gt[n][best_idx[n][idx].long()] if gcount[n] > 0 else 0.0
        r_idx[rows] = idx
    return rois, r_cls, r_gt, r_idx

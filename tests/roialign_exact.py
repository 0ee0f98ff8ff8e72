"""Operands and a plain fp64 reference for the kernel-level tests of RoIAlign (csrc/roi.hip): separable and vector forward, scatter
backward, one-row and two-row gather backward.

The reference restates torchvision roi_align (aligned=True, sampling_ratio=0) under the ROIPooler level rule, sample by sample, in fp64
on the fp32 boxes.  The sample grid of a bin is a product grid and a sample is dead when either coordinate is, so the walk runs once per
axis: `axis_walk` visits every sample row (column) of every bin row (column), applies the dead test, the clamps and the two taps, and
leaves the summed tap weights per (bin, pixel); forward and backward contract those with the map (the pooled gradient) in fp64.  The level
comes from oracle.d2_rcnn.assign_levels on the fp32 boxes: it is part of the specification.  A box with x2 <= x1 or y2 <= y1, or a row
with image index -1, pools to zero and receives no gradient.

The same walk returns the facts the kernels branch on (`walk`: footprint, sample coordinates, run of pixels under a bin column, run of bin
rows on a feature row; `candidates`: what a gather workgroup's bounding-box test lets through), so the tests can assert their own coverage.

Two kinds of check, as in detr_kernel_refs.py:

  lattice cases   every level coordinate (box * scale - 0.5) is a multiple of 1/8, rw / P and rh / P are multiples of 1/8, the adaptive
                  grids gh, gw are powers of two, features and pooled gradients are small integers.  Every weight, product and partial
                  sum is then exact in fp32 in any order, with or without FMA, and 1 / count is a power of two: a kernel is held to
                  torch.equal.  `check_lattice` verifies that budget per output element instead of assuming it.
  bounded case    random boxes (grids of 3, 5, ...): a kernel may be FACTOR times as far from the fp64 reference as the oracle's own fp32
                  roi_pool / autograd on the same operands.

Nothing here touches the library under test.  Shared by test_roialign_exact_cpu.py and test_roialign_exact_gpu.py."""
import functools
import math

import torch

SCALES = (1 / 4, 1 / 8, 1 / 16, 1 / 32)
STRIDES = (4, 8, 16, 32)
C = 256
SEG = 32                       # pixels of a gather workgroup's segment
CHUNK = 256                    # rows a gather workgroup scans at a time
FACTOR = 8.0
MUTANTS = ("dead_ge", "no_clamp", "no_hi", "short", "level")


# ------------------------------------------------------------------------------------------------ the walk
def degenerate(rois):
    return ~((rois[:, 3] > rois[:, 1]) & (rois[:, 4] > rois[:, 2]))


def assign_levels(rois):
    """oracle.d2_rcnn.assign_levels on the fp32 boxes; 0 where the box is degenerate (its level does not matter: it pools to zero)"""
    from oracle.d2_rcnn import assign_levels as al
    lv = al(rois[:, 1:5].float())
    return torch.where(degenerate(rois), torch.zeros_like(lv), lv)


def axis_walk(a1, a2, size, P, mut=None):
    """one axis of one ROI: (grid, [(bin, coordinate, dead)], weights (P, size) fp64, taps (P, size): how many samples touch the pixel)"""
    r = a2 - a1
    b = r / P
    g = math.ceil(r / P)
    Wm = torch.zeros(P, size, dtype=torch.float64)
    Nm = torch.zeros(P, size, dtype=torch.float64)
    samples = []
    for p in range(P):
        for i in range(g):
            v = a1 + p * b + (i + 0.5) * b / g
            dead = (v <= -1.0 or v >= size) if mut == "dead_ge" else (v < -1.0 or v > size)
            samples.append((p, v, dead))
            if dead:
                continue
            v = max(v, 0.0)
            lo = int(v)
            if mut == "no_clamp":
                hi = lo + 1
            elif lo >= size - 1:
                hi = lo = size - 1
                v = float(lo)
            else:
                hi = lo + 1
            l = v - lo
            h = 1.0 - l
            if lo < size:
                Wm[p, lo] += h
                Nm[p, lo] += 1
            if hi < size and mut != "no_hi":
                Wm[p, hi] += l
                Nm[p, hi] += hi != lo
    return g, samples, Wm, Nm


def _extent(Wm):
    nz = (Wm != 0).any(0).nonzero().flatten()
    return (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (0, 0)


def walk(rois, shapes, P, mut=None):
    """per ROI: level, image, grids, samples, tap weights and the facts the kernels branch on"""
    lv = assign_levels(rois)
    if mut == "level":
        lv = (lv + 1).clamp(max=3)
    deg = degenerate(rois)
    out = []
    for r in range(len(rois)):
        b, l = int(rois[r, 0]), int(lv[r])
        H, W = shapes[l]
        x1, y1, x2, y2 = (float(v) * SCALES[l] - 0.5 for v in rois[r, 1:5].tolist())
        f = dict(b=b, level=l, zero=bool(deg[r]) or b < 0, x1=x1, y1=y1, x2=x2, y2=y2, H=H, W=W)
        if f["zero"]:
            f.update(gh=0, gw=0, ys=[], xs=[], RW=torch.zeros(P, H, dtype=torch.float64), CW=torch.zeros(P, W, dtype=torch.float64))
            f.update(RN=f["RW"].clone(), CN=f["CW"].clone())
        else:
            f["gh"], f["ys"], f["RW"], f["RN"] = axis_walk(y1, y2, H, P, mut)
            f["gw"], f["xs"], f["CW"], f["CN"] = axis_walk(x1, x2, W, P, mut)
            if mut == "short" and _extent(f["RW"])[1] > 0:
                f["RW"][:, _extent(f["RW"])[1] - 1] = 0
        f["count"] = max(f["gh"] * f["gw"], 1)
        f["yext"], f["xext"] = _extent(f["RW"]), _extent(f["CW"])
        # the kernels' footprint (forward tables, gather candidate test)
        f["fy"] = (min(max(math.floor(y1) - 1, 0), H - 1), min(max(math.floor(y2) + 2, 0), H - 1))
        f["fx"] = (min(max(math.floor(x1) - 1, 0), W - 1), min(max(math.floor(x2) + 2, 0), W - 1))
        runs = []
        for p in range(P):
            nz = (f["CW"][p] != 0).nonzero().flatten()
            runs.append(int(nz[-1]) - int(nz[0]) + 1 if len(nz) else 0)
        f["col_runs"] = runs
        f["wave_maxrun"] = [max(runs[2 * w:2 * w + 2]) for w in range((P + 1) // 2)]      # a wave of the separable forward holds two bin columns
        rr = {}
        for y in range(*f["yext"]):
            nz = (f["RW"][:, y] != 0).nonzero().flatten()
            if len(nz):
                rr[y] = int(nz[-1]) - int(nz[0]) + 1
        f["row_runs"] = rr
        out.append(f)
    return out


def ref_forward(feats, rois, P, mut=None, facts=None):
    """feats: four (N, H, W, C) maps -> pooled (R, P, P, C) fp64"""
    facts = facts if facts is not None else walk(rois, [t.shape[1:3] for t in feats], P, mut)
    out = torch.zeros(len(rois), P, P, feats[0].shape[3], dtype=torch.float64)
    for r, f in enumerate(facts):
        (y0, y1), (x0, x1) = f["yext"], f["xext"]
        if f["zero"] or y1 == y0 or x1 == x0:
            continue
        F = feats[f["level"]][f["b"], y0:y1, x0:x1].double()
        T = torch.einsum("qx,yxc->yqc", f["CW"][:, x0:x1], F)
        out[r] = torch.einsum("py,yqc->pqc", f["RW"][:, y0:y1], T) / f["count"]
    return out


def ref_backward(shapes, N, rois, P, gp, mut=None, facts=None):
    """gp: (R, P, P, C) pooled gradient -> four (N, H, W, C) gradient maps fp64"""
    facts = facts if facts is not None else walk(rois, shapes, P, mut)
    G = [torch.zeros(N, h, w, gp.shape[3], dtype=torch.float64) for h, w in shapes]
    for r, f in enumerate(facts):
        (y0, y1), (x0, x1) = f["yext"], f["xext"]
        if f["zero"] or y1 == y0 or x1 == x0:
            continue
        T = torch.einsum("py,pqc->yqc", f["RW"][:, y0:y1], gp[r].double())
        G[f["level"]][f["b"], y0:y1, x0:x1] += torch.einsum("qx,yqc->yxc", f["CW"][:, x0:x1], T) / f["count"]
    return G


def candidates(rois, shapes, N, P, rows, rois_sorted):
    """what the gather kernels' bounding-box test lets through: per level a tensor (N, row groups, segments, chunks) of counts.
    rows = 1 (one-row kernel) or 2 (two-row kernel); chunks count from the image's first row when the rows are sorted by image."""
    facts = walk(rois, shapes, P)
    R = len(rois)
    nch = (R + CHUNK - 1) // CHUNK
    cnt = [torch.zeros(N, (h + rows - 1) // rows, (w + SEG - 1) // SEG, nch, dtype=torch.int64) for h, w in shapes]
    first = {}
    for r, f in enumerate(facts):
        first.setdefault(f["b"], r)
    for r, f in enumerate(facts):
        if f["b"] < 0:
            continue
        ch = (r - first[f["b"]]) // CHUNK if rois_sorted else r // CHUNK
        (r0, r1), (c0, c1) = f["fy"], f["fx"]
        if r1 >= r0 and c1 >= c0:
            cnt[f["level"]][f["b"], r0 // rows:r1 // rows + 1, c0 // SEG:c1 // SEG + 1, ch] += 1
    return cnt


# ------------------------------------------------------------------------------------------------ lattice cases
class Case:
    def __init__(self, name, shapes, N, P, rois, levels=None, rois_sorted=False, pad_at=None, const_levels=False, free_y=False, coarse=False, seed=0):
        self.name, self.shapes, self.N, self.P = name, [tuple(s) for s in shapes], N, P
        self.rois = torch.tensor(rois, dtype=torch.float32).reshape(-1, 5)
        self.levels = levels                          # the level each row was built for (None: not asserted, e.g. a degenerate box)
        self.rois_sorted, self.pad_at, self.const_levels, self.free_y, self.coarse, self.seed = rois_sorted, pad_at, const_levels, free_y, coarse, seed

    @property
    def R(self):
        return len(self.rois)

    def forward_rois(self):
        """the rows the forward runs: a padding row (image index -1, a box that would pool non-zero values) between valid rows"""
        if self.pad_at is None:
            return self.rois
        pad = torch.tensor([[-1.0, 8.0, 8.0, 40.0, 40.0]])
        return torch.cat([self.rois[:self.pad_at], pad, self.rois[self.pad_at:]])


def lbox(b, l, x1, y1, w, h):
    """a row whose box has the level coordinates (x1, y1, x1 + w, y1 + h) on level l"""
    s = STRIDES[l]
    return [float(b), (x1 + 0.5) * s, (y1 + 0.5) * s, (x1 + w + 0.5) * s, (y1 + h + 0.5) * s]


RAGGED = ((51, 67), (26, 34), (13, 17), (7, 9))


def _edges():
    H, W = RAGGED[0]
    rows, lv = [], []

    def add(row, l=0):
        rows.append(row); lv.append(l)
    for b, x1, y1 in ((0, -1.5, -1.5),                 # samples exactly at -1 (alive), 0, integers; top-left corner of image 0
                      (0, -1.625, -1.625),             # first sample at -1.125 (dead)
                      (1, W - 6.5, H - 6.5),           # last sample exactly at W / H (alive), one exactly at W - 1 / H - 1; bottom-right corner
                      (1, W - 6.375, H - 6.375),       # last sample at W + 0.125 / H + 0.125 (dead)
                      (0, W - 7.0, H - 7.0),           # samples at x.5, the last in (W - 1, W]: both taps on the last pixel
                      (1, W - 6.5, -1.5),              # top-right corner
                      (0, -1.5, H - 6.5),              # bottom-left corner
                      (0, 10.5, 20.5), (1, 10.0, 20.0), (0, -0.5, -0.5),     # interior on integers, at x.5; first sample exactly at 0
                      (0, -12.0, 10.0), (0, W + 3.0, 10.0), (1, 10.0, -12.0), (1, 10.0, H + 3.0)):    # entirely outside on each side
        add(lbox(b, 0, x1, y1, 7.0, 7.0))
    add(lbox(0, 0, -4.5, -4.5, 24.5, 24.5))            # bins of 3.5 over the top-left corner of image 0
    add(lbox(1, 0, W - 10.0, H - 12.0, 24.5, 24.5))
    add(lbox(0, 1, -3.5, -2.0, 14.0, 14.0), 1)
    add(lbox(1, 1, 25.0, 18.0, 14.0, 14.0), 1)
    add(lbox(0, 2, 5.0, -4.0, 24.5, 10.5), 2)
    add(lbox(1, 2, -6.25, 4.5, 14.0, 14.0), 2)
    add(lbox(1, 3, -2.5, -3.5, 14.0, 14.0), 3)         # covers the whole 7 x 9 map
    add(lbox(0, 3, 4.0, 2.0, 24.5, 24.5), 3)
    return Case("edges", RAGGED, 2, 7, rows, lv, seed=1)


def _degenerate():
    rows = [lbox(0, 0, 5.0, 5.0, 7.0, 7.0),
            lbox(0, 0, 10.0, 10.0, 0.0, 7.0),          # zero width
            lbox(1, 0, 10.0, 10.0, 7.0, 0.0),          # zero height
            lbox(0, 0, 30.0, 10.0, -14.0, 7.0),        # negative width, positive height: the footprint's column count is negative
            lbox(0, 0, 3.0, -1.5, -14.0, 7.0),         # the same at the top-left corner of image 0
            lbox(1, 0, 30.0, 20.0, -0.25, 7.0),
            lbox(1, 0, 10.0, 30.0, 7.0, -14.0),        # positive width, negative height
            lbox(0, 0, 30.0, 30.0, -7.0, -7.0),        # both negative: the area is positive, the level rule sees a normal box
            lbox(1, 1, 20.0, 20.0, -14.0, -14.0),
            lbox(1, 0, 40.0, 30.0, 10.5, 10.5)]
    return Case("degenerate", RAGGED, 2, 7, rows, None, pad_at=2, seed=2)


def _bins():
    rows = [lbox(0, 0, 10.125, 20.0, 1.75, 1.75),      # bins of 0.25: seven bin rows on one feature row
            lbox(0, 0, 5.0, 7.5, 1.75, 1.75),
            lbox(0, 0, 30.5, 3.5, 7.0, 7.0), lbox(0, 0, 30.0, 12.0, 7.0, 7.0), lbox(0, 0, 20.25, 12.25, 7.0, 7.0),   # bins of 1
            lbox(0, 0, 3.25, 40.5, 10.5, 10.5), lbox(0, 0, 16.0, 44.5, 10.5, 10.5),                                # 1.5
            lbox(0, 0, 20.0, 30.0, 24.5, 24.5), lbox(0, 0, 2.5, 2.5, 24.5, 24.5),                                  # 3.5
            lbox(0, 0, -8.0, 50.0, 52.5, 1.75),        # bin columns of 7.5 pixels: the separable forward's generic loop
            lbox(0, 0, 40.0, 3.0, 1.75, 52.5),         # bin rows of 7.5 pixels
            lbox(0, 0, -3.0, 58.0, 52.5, 1.75), lbox(0, 0, -4.0, 61.0, 52.5, 1.75), lbox(0, 0, -2.0, 55.0, 52.5, 1.75),   # the map's edge cuts the last bin column to 6, 7, 5 pixels
            lbox(0, 0, 6.0, 26.0, 28.0, 3.5), lbox(0, 0, 6.5, 36.5, 28.0, 3.5),                                       # 4
            lbox(0, 0, 1.0, 1.0, 14.0, 14.0), lbox(0, 0, 1.5, 20.5, 14.0, 14.0)]                                      # 2
    lv = [0] * len(rows)
    rows.append(lbox(0, 3, -20.0, -20.0, 52.5, 52.5)); lv.append(3)
    return Case("bins", ((64, 48), (32, 24), (16, 12), (8, 6)), 1, 7, rows, lv, seed=3)


def _mixed(P):
    H, W = RAGGED[0]
    side = {1: 16.0, 2: 16.0, 5: 20.0, 7: 14.0}[P]    # bins of 16, 8, 4, 2 on the coarse levels (an area of at least 14^2 level pixels)
    rows = [lbox(0, 0, -1.5, -1.5, 1.0 * P, 1.0 * P),
            lbox(1, 0, 5.125, 9.0, 0.25 * P, 0.25 * P),
            lbox(0, 0, 20.0, 30.0, 3.5 * P, 3.5 * P),
            lbox(1, 0, W - 4.0, H - 3.5, 1.5 * P, 1.5 * P),
            lbox(0, 0, 3.0, 3.0, 7.5 * P, 0.25 * P),
            lbox(1, 0, 50.0, 2.5, 0.25 * P, 7.5 * P)]
    lv = [0] * 6
    for l in (1, 2, 3):
        rows.append(lbox(l % 2, l, 2.0 - l, 2.5 - 2 * l, side, side)); lv.append(l)
    return Case(f"mixed_P{P}", RAGGED, 2, P, rows, lv, seed=10 + P)


def _tall(name, shape):
    H, W = shape
    small = ((4, 4), (4, 4), (4, 4))
    if H > W:
        rows = [lbox(0, 0, 2.0, -8.0, 1.75, 224.0), lbox(0, 0, -1.5, H - 6.5, 7.0, 7.0)]       # bins of 32 rows: the footprint is every row of the map
    else:
        rows = [lbox(0, 0, -50.0, -0.5, 448.0, 0.875), lbox(0, 0, W - 6.5, -1.5, 7.0, 7.0)]    # bins of 64 columns
    return Case(name, (shape,) + small, 1, 7, rows, [0, 0], seed=20)


def _levels():
    rows, lv = [], []
    for k, T in enumerate((112.0, 224.0, 448.0)):
        for d in (-1, 0, 1):
            # width 2 T, height T / 2 * (1 + d * 2^-15): sqrt(area) = T * (1 + d * 2^-16) to first order.  On the level the rule must
            # choose the bins are 4 (8) pixels wide and 1 + 2^-15, 1 (2 - 2^-14) pixels high: the grids are powers of two.  The box ends at
            # the image's top edge, so its live sample rows lie in [-1, 0]: clamped to 0, weight exactly 1 on row 0, no y fraction at all.
            h = T / 2 * (1 + d * 2.0 ** -15)
            rows.append([0.0, 8.0, -h, 8.0 + 2 * T, 0.0])
            lv.append(k + (d >= 0))
    return Case("levels", ((8, 64),) * 4, 1, 7, rows, lv, const_levels=True, free_y=True, seed=30)


def _scan():
    """N = 4, rows sorted by image; images 0 and 2 have no ROI, image 1 has 257 (two scan chunks), image 3 one.  Coordinates in halves, grids
    of 1 (bins of 1) or 2 x 2 (bins of 2), so hundreds of ROIs on one pixel stay inside the exactness budget."""
    g = torch.Generator().manual_seed(40)
    rows = []
    for _ in range(250):                               # a pile in segment 0, rows 0 .. 12
        x1 = -0.5 + 0.5 * int(torch.randint(0, 21, (1,), generator=g))
        y1 = -0.5 + 0.5 * int(torch.randint(0, 8, (1,), generator=g))
        rows.append(lbox(1, 0, x1, y1, 7.0, 7.0))
    rows.append(lbox(1, 0, 40.0, 16.0, 7.0, 7.0))                                         # alone in segment 1
    rows += [lbox(1, 0, 40.0, 32.0, 7.0, 7.0), lbox(1, 0, 42.5, 33.0, 7.0, 7.0)]        # two in segment 1
    rows += [lbox(1, 0, 3.0, 32.0, 7.0, 7.0), lbox(1, 0, 5.5, 33.5, 7.0, 7.0), lbox(1, 0, 8.0, 33.0, 7.0, 7.0)]     # three in segment 0
    rows.append(lbox(1, 0, 4.0, 2.5, 7.0, 7.0))                                           # row 257 of image 1 (second chunk), on the pile
    rows.append(lbox(3, 1, 3.0, 3.0, 14.0, 14.0))
    return Case("scan", ((48, 70), (24, 35), (12, 18), (6, 9)), 4, 7, rows, [0] * 257 + [1], rois_sorted=True, coarse=True, seed=40)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [_edges(), _degenerate(), _bins(), _mixed(1), _mixed(2), _mixed(5), _mixed(7),
          _tall("sep_208x8", (208, 8)), _tall("vec_209x8", (209, 8)), _tall("vec_2x345", (2, 345)), _levels(), _scan()]
    return {c.name: c for c in cs}


CASE_NAMES = ("edges", "degenerate", "bins", "mixed_P1", "mixed_P2", "mixed_P5", "mixed_P7", "sep_208x8", "vec_209x8", "vec_2x345", "levels", "scan")


@functools.lru_cache(maxsize=None)
def operands(name):
    """(feats fp32 NHWC: integers of magnitude 1 .. 4, or the constant l + 1 on level l; pooled gradient for case.rois: integers of magnitude 1, 2)"""
    c = cases()[name]
    g = torch.Generator().manual_seed(c.seed)

    def ints(shape, hi):
        return (torch.randint(1, hi + 1, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()
    if c.const_levels:
        feats = [torch.full((c.N, h, w, C), float(l + 1)) for l, (h, w) in enumerate(c.shapes)]
    else:
        feats = [ints((c.N, h, w, C), 4) for h, w in c.shapes]
    return feats, ints((c.R, c.P, c.P, C), 2)


@functools.lru_cache(maxsize=None)
def facts(name, fwd=False):
    c = cases()[name]
    return walk(c.forward_rois() if fwd else c.rois, c.shapes, c.P)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pooled for case.forward_rois(), gradient maps for case.rois), fp64; computed once, shared by the tests, never modified"""
    c = cases()[name]
    feats, gp = operands(name)
    return ref_forward(feats, c.forward_rois(), c.P, facts=facts(name, True)), ref_backward(c.shapes, c.N, c.rois, c.P, gp, facts=facts(name))


def _granularity(t):
    """the largest power of two that divides every entry of t"""
    for k in range(0, 40):
        s = t * 2.0 ** k
        if bool((s == s.round()).all()):
            return 2.0 ** -k
    raise AssertionError("not dyadic within 2^-39")


def _pow2(n):
    return n >= 1 and n & (n - 1) == 0


def check_lattice(name):
    """the preconditions of exactness, and the budget: for every output element sum |terms| < 2^24 * (granularity of a term).  Every partial sum
    in any order is then a multiple of the granularity below 2^24 of them: representable in fp32.  Returns the worst budget use (< 1)."""
    c = cases()[name]
    feats, gp = operands(name)
    assert all(torch.equal(t, t.bfloat16().float()) and torch.equal(t, t.round()) for t in feats + [gp])
    lv = assign_levels(c.rois)
    use_f = 0.0
    A = [torch.zeros(c.N, h, w, dtype=torch.float64) for h, w in c.shapes]
    gran = [math.inf] * 4
    for r, f in enumerate(facts(name)):
        if c.levels is not None:
            assert int(lv[r]) == c.levels[r], (name, r, int(lv[r]), c.levels[r])
        if f["zero"]:
            continue
        assert _pow2(f["gh"]) and _pow2(f["gw"]), (name, r, f["gh"], f["gw"])
        unit = 0.5 if c.coarse else 0.125
        coords = [f["x1"], f["x2"], (f["x2"] - f["x1"]) / c.P]
        if c.free_y:
            assert all(dead or -1.0 <= v <= 0.0 for _, v, dead in f["ys"]) and any(not dead for _, v, dead in f["ys"])
        else:
            coords += [f["y1"], f["y2"], (f["y2"] - f["y1"]) / c.P]
        assert all(v / unit == round(v / unit) for v in coords), (name, r, coords)
        if c.coarse:
            assert f["count"] in (1, 4)
        (y0, y1), (x0, x1) = f["yext"], f["xext"]
        if y1 == y0 or x1 == x0:
            continue
        gy, gx = _granularity(f["RW"]), _granularity(f["CW"])
        if c.coarse:
            assert gy >= 0.5 and gx >= 0.5
        # forward: terms wy * wx * feature (granularity gy * gx); 1 / count is a power of two
        F = feats[f["level"]][f["b"], y0:y1, x0:x1].double().abs().amax(-1)
        s = torch.einsum("py,qx,yx->pq", f["RW"][:, y0:y1], f["CW"][:, x0:x1], F).max().item()
        use_f = max(use_f, s / (2.0 ** 24 * gy * gx))
        # backward: terms wy * wx * g / count, summed over every ROI that touches the pixel
        gm = gp[r].double().abs().amax(-1)
        A[f["level"]][f["b"], y0:y1, x0:x1] += torch.einsum("py,qx,pq->yx", f["RW"][:, y0:y1], f["CW"][:, x0:x1], gm) / f["count"]
        gran[f["level"]] = min(gran[f["level"]], gy * gx / f["count"])
    use_b = max((a.max().item() / (2.0 ** 24 * q) for a, q in zip(A, gran) if q < math.inf), default=0.0)
    assert use_f < 1.0 and use_b < 1.0, (name, use_f, use_b)
    return use_f, use_b


# ------------------------------------------------------------------------------------------------ the bounded case
BOUNDED_SHAPES = ((96, 128), (48, 64), (24, 32), (12, 16))       # a 512 x 384 image


@functools.lru_cache(maxsize=None)
def bounded_case():
    """40 random boxes on all four levels and four with bins of exactly 3 and 7 pixels (grids of 3, 5, ... : nothing dyadic), some overhanging the image; bf16-representable features
    and pooled gradients.  Returns the operands, the fp64 reference and the oracle's fp32 roi_pool / autograd on the same operands."""
    from oracle import d2_rcnn as d2
    g = torch.Generator().manual_seed(77)
    N, P, IW, IH = 2, 7, 512.0, 384.0
    per = []
    for lo, hi in ((8.0, 100.0), (115.0, 215.0), (230.0, 430.0), (455.0, 700.0)):
        s = lo + (hi - lo) * torch.rand(10, generator=g)           # sqrt(area)
        a = torch.exp((torch.rand(10, generator=g) - 0.5) * 1.2)   # aspect
        w, h = s * a, s / a
        cx = IW * (torch.rand(10, generator=g) * 1.2 - 0.1)
        cy = IH * (torch.rand(10, generator=g) * 1.2 - 0.1)
        per.append(torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1))
    boxes = torch.cat(per).float()
    img = (torch.arange(40) % N).float()
    # bins of exactly 3 and 7 pixels (grids of 3 and 7: 1 / count is not a power of two, so they cannot be lattice cases)
    extra = torch.tensor([lbox(0, 0, 10.25, 20.5, 21.0, 21.0), lbox(1, 0, 30.0, 5.0, 49.0, 10.5), lbox(0, 1, 3.125, 2.25, 21.0, 21.0), lbox(1, 3, -5.0, -4.0, 49.0, 49.0)])
    boxes, img = torch.cat([boxes, extra[:, 1:]]), torch.cat([img, extra[:, 0]])
    order = torch.argsort(img, stable=True)
    rois = torch.cat([img[:, None], boxes], 1)[order].contiguous()
    feats = [torch.randn(N, h, w, C, generator=g).bfloat16().float() for h, w in BOUNDED_SHAPES]
    gp = torch.randn(len(rois), P, P, C, generator=g).bfloat16().float()
    fc = walk(rois, BOUNDED_SHAPES, P)
    out64 = ref_forward(feats, rois, P, facts=fc)
    G64 = ref_backward(BOUNDED_SHAPES, N, rois, P, gp, facts=fc)
    fr = [f.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for f in feats]
    out32 = d2.roi_pool(d2.make_cfg(num_classes=8), fr, [rois[rois[:, 0] == i, 1:] for i in range(N)])
    out32.backward(gp.permute(0, 3, 1, 2).contiguous())
    G32 = [f.grad.permute(0, 2, 3, 1).contiguous() for f in fr]
    return dict(N=N, P=P, rois=rois, feats=feats, gp=gp, facts=fc, out64=out64, G64=G64, out32=out32.detach().permute(0, 2, 3, 1).contiguous(), G32=G32)


def bf16_half_ulp(ref):
    """half a bf16 ulp of each reference value (8 significant bits: ulp = 2^(e - 7) for 2^e <= |v| < 2^(e + 1))"""
    e = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126)))
    return 2.0 ** (e - 8)


def bound(got, r32, r64, lowp=False):
    """(worst err_kernel / allowed, err_ref32, ratio err_kernel / err_ref32).  allowed = FACTOR * max|ref32 - ref64| (+ half a bf16 ulp of the
    reference value for a bf16 output)"""
    got, r64 = got.detach().cpu().double(), r64.double()
    e32 = (r32.double() - r64).abs().max().item()
    err = (got - r64).abs()
    if lowp:
        err = (err - bf16_half_ulp(r64)).clamp(min=0)
    ek = err.max().item()
    return ek <= FACTOR * e32 and bool(torch.isfinite(got).all()), ek, e32

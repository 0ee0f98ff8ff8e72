"""Operands and references for the exact tests of the sparse RPN-head backward (csrc/rpn_sparse.hip: aldi_rpn_active_pixels,
aldi_rpn_sparse_gather, aldi_rpn_sparse_scatter).  CPU only: test_rpn_sparse_exact_cpu.py pins what is here without a GPU (the scatter
reference against torch.autograd of the dense 3x3 convolution, which fixes the tap orientation independently of the kernel),
test_rpn_sparse_exact_gpu.py compares the three entry points with it bit for bit.

A tiny five-level pyramid, two images.  A ROW is a pixel position: levels first, then images, then h, w -- row0[l] = N * sum_{k<l} H_k W_k.
Level 0 alone has 4160 rows, more than one 4096-row segment of the list kernels; 5200 and the later level boundaries fall inside a 64-row
ballot word.  Every per-level tensor here is a view of one flat [rows, channels] tensor, which is also how the tests hand them to the
device (five pointers into one buffer)."""
from typing import List, Sequence, Tuple

import torch

LEVELS = [(40, 52), (20, 26), (3, 4), (2, 2), (1, 1)]
N = 2
CH = 16                                    # head channels (objectness + deltas, padded)
ROW0 = [0]
for _h, _w in LEVELS:
    ROW0.append(ROW0[-1] + N * _h * _w)
TOTAL = ROW0[-1]                           # 5234
SEG = 4096                                 # rows per segment of the list kernels


def row_of(l: int, n: int, h: int, w: int) -> int:
    H, W = LEVELS[l]
    assert 0 <= n < N and 0 <= h < H and 0 <= w < W
    return ROW0[l] + (n * H + h) * W + w


def pixel_of(row: int) -> Tuple[int, int, int, int]:
    l = max(k for k in range(len(LEVELS)) if row >= ROW0[k])
    H, W = LEVELS[l]
    r = row - ROW0[l]
    return l, r // (H * W), (r % (H * W)) // W, r % W


def level_views(flat: torch.Tensor) -> List[torch.Tensor]:
    """[TOTAL, C] -> five [N, H, W, C] views"""
    assert flat.shape[0] == TOTAL and flat.is_contiguous()
    return [flat[ROW0[l]:ROW0[l + 1]].view(N, H, W, flat.shape[1]) for l, (H, W) in enumerate(LEVELS)]


# ------------------------------------------------------------------------------------------------
# active list
# ------------------------------------------------------------------------------------------------
BOUNDARY_ROWS = sorted({r for b in ROW0[1:-1] + [SEG] for r in (b - 1, b)})
ACTIVE_PATTERNS = ("none", "all", "first", "last", "last_channel", "neg_zero", "nan", "denormal", "boundaries")


def ghead_pattern(kind: str) -> torch.Tensor:
    """fp32 [TOTAL, CH] head gradient"""
    g = torch.zeros(TOTAL, CH)
    if kind == "none":
        pass
    elif kind == "all":
        g[:, 0] = 1.0
        g[::3, 0], g[::3, 7] = 0.0, -2.0
    elif kind == "first":
        g[0, 5] = 1.0
    elif kind == "last":
        g[TOTAL - 1, 0] = -1.0
    elif kind == "last_channel":
        g[[3, 64, 4095, 4160, 5201], CH - 1] = 0.5
    elif kind == "neg_zero":
        g[[0, 7, 4100, TOTAL - 1]] = -0.0
        g[9, 3] = -0.0
    elif kind == "nan":
        g[4101, 3] = float("nan")
    elif kind == "denormal":
        g[70, 2], g[5233, 15] = 1e-40, -1.4e-45
    elif kind == "boundaries":
        g[BOUNDARY_ROWS, 1] = 1.0
    else:
        raise KeyError(kind)
    return g


def active_ref(ghead: torch.Tensor) -> torch.Tensor:
    """ascending rows with any non-zero channel (-0.0 is zero, a NaN is not), int64"""
    return torch.nonzero((ghead != 0).any(dim=1)).squeeze(1)


# ------------------------------------------------------------------------------------------------
# the pixels of the gather and scatter tests
# ------------------------------------------------------------------------------------------------
def pixel_rows() -> List[int]:
    """ascending rows: on the large level isolated pixels, horizontal / vertical / diagonal / anti-diagonal pairs, a full 3 x 3 block, the
    four corners and a pixel on each edge; a corner and an edge of level 1; EVERY pixel of the 3 x 4 and 2 x 2 levels in both images (so
    that targets are reached through up to nine taps and every owner case of the scatter occurs); the 1 x 1 level in image 1 only (eight of
    its taps are outside).  Image 0's last pixel and image 1's first are neighbouring rows and must not see each other."""
    px = [(0, 0, 5, 5), (0, 0, 10, 10), (0, 0, 10, 11), (0, 0, 15, 20), (0, 0, 16, 20), (0, 0, 20, 30), (0, 0, 21, 31), (0, 0, 25, 10), (0, 0, 26, 9),
          (0, 0, 0, 0), (0, 0, 0, 51), (0, 0, 39, 0), (0, 0, 39, 51), (0, 0, 0, 20), (0, 0, 39, 21), (0, 0, 20, 0), (0, 0, 22, 51),
          (0, 1, 0, 0), (0, 1, 39, 51)] + [(0, 1, h, w) for h in (30, 31, 32) for w in (40, 41, 42)]
    px += [(1, 0, 19, 25), (1, 0, 0, 25), (1, 1, 10, 13)]
    px += [(2, n, h, w) for n in range(N) for h in range(3) for w in range(4)]
    px += [(3, n, h, w) for n in range(N) for h in range(2) for w in range(2)]
    px += [(4, 1, 0, 0)]
    rows = sorted(row_of(*p) for p in px)
    assert len(set(rows)) == len(rows)
    return rows


def tap_offset(tap: int) -> Tuple[int, int]:
    return tap // 3 - 1, tap % 3 - 1


# ------------------------------------------------------------------------------------------------
# gather
# ------------------------------------------------------------------------------------------------
def random_bits(shape: Sequence[int], dtype: torch.dtype, seed: int) -> torch.Tensor:
    """every bit pattern, NaN payloads and infinities included: the gather copies bits"""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bfloat16:
        return torch.randint(-32768, 32768, tuple(shape), generator=g, dtype=torch.int16).view(torch.bfloat16)
    return torch.randint(-2 ** 31, 2 ** 31, tuple(shape), generator=g, dtype=torch.int32).view(torch.float32)


def as_int(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def gather_ref(rows: Sequence[int], cap: int, ghead: torch.Tensor, hidden: torch.Tensor, feat: torch.Tensor):
    """(G [cap, CH], Tm [cap, Cf], X9 [cap, 9, Cf]) in hidden's dtype: G the head-gradient row as torch converts it, Tm and X9 bit copies,
    zeros for taps outside the level and for the rows from len(rows) to cap"""
    T, Cf = hidden.dtype, hidden.shape[1]
    G, Tm, X9 = torch.zeros(cap, CH, dtype=T), torch.zeros(cap, Cf, dtype=T), torch.zeros(cap, 9, Cf, dtype=T)
    for s, row in enumerate(rows):
        l, n, h, w = pixel_of(row)
        H, W = LEVELS[l]
        G[s], Tm[s] = ghead[row].to(T), hidden[row]
        for tap in range(9):
            dh, dw = tap_offset(tap)
            if 0 <= h + dh < H and 0 <= w + dw < W:
                X9[s, tap] = feat[row_of(l, n, h + dh, w + dw)]
    return G, Tm, X9


# ------------------------------------------------------------------------------------------------
# scatter
# ------------------------------------------------------------------------------------------------
def scatter_delta(rows: Sequence[int], Y: torch.Tensor, *, sign: int = 1):
    """the definition: delta[t] = sum over taps of Y[slot(t - d(tap))][tap], i.e. the active pixel q adds Y[slot(q)][tap] to the target
    q + d(tap) where that is inside q's level and image.  fp64 [TOTAL, Cf] and the bool [TOTAL] of targets reached.  sign = -1 is the
    WRONG variant with the tap offset of the opposite sign."""
    Yd = Y.double()
    delta, reached = torch.zeros(TOTAL, Y.shape[2], dtype=torch.float64), torch.zeros(TOTAL, dtype=torch.bool)
    for s, row in enumerate(rows):
        l, n, h, w = pixel_of(row)
        H, W = LEVELS[l]
        for tap in range(9):
            dh, dw = tap_offset(tap)
            th, tw = h + sign * dh, w + sign * dw
            if 0 <= th < H and 0 <= tw < W:
                t = row_of(l, n, th, tw)
                delta[t] += Yd[s, tap]
                reached[t] = True
    return delta, reached


def scatter_ref(rows: Sequence[int], Y: torch.Tensor, prefill: torch.Tensor, *, round_each: bool = False) -> torch.Tensor:
    """prefill + delta in prefill's dtype: the exact sum (asserted to be exact in fp32) rounded ONCE to nearest-even.  round_each is the
    WRONG variant that rounds the map after every contribution."""
    T = prefill.dtype
    if round_each:
        out = prefill.clone()
        for s, row in enumerate(rows):
            l, n, h, w = pixel_of(row)
            H, W = LEVELS[l]
            for tap in range(9):
                dh, dw = tap_offset(tap)
                if 0 <= h + dh < H and 0 <= w + dw < W:
                    t = row_of(l, n, h + dh, w + dw)
                    out[t] = (out[t].double() + Y[s, tap].double()).float().to(T)
        return out
    exact = prefill.double() + scatter_delta(rows, Y)[0]
    assert torch.equal(exact.float().double(), exact)
    return exact.float().to(T)


def y_exact(cap: int, count: int, Cf: int, dtype: torch.dtype) -> torch.Tensor:
    """[cap, 9, Cf] integers in [-2, 2] that differ by slot, tap and channel; the rows past the count hold 77 and must not be read"""
    s, tap, c = torch.arange(cap)[:, None, None], torch.arange(9)[None, :, None], torch.arange(Cf)[None, None, :]
    y = ((s * 7 + tap * 3 + c) % 5 - 2).float()
    y[count:] = 77.0
    return y.to(dtype)


def prefill_exact(Cf: int, dtype: torch.dtype) -> torch.Tensor:
    """[TOTAL, Cf] integers in [-5, 5]"""
    return (((torch.arange(TOTAL)[:, None] + torch.arange(Cf)[None, :]) % 11) - 5).float().to(dtype)


def y_ones(cap: int, count: int, Cf: int) -> torch.Tensor:
    y = torch.ones(cap, 9, Cf)
    y[count:] = 77.0
    return y.to(torch.bfloat16)


def prefill_ties(Cf: int) -> torch.Tensor:
    """bf16 [TOTAL, Cf]: 248 + channel % 4.  A pixel of the fully active 3 x 4 level that nine neighbours reach ends at 257, 258, 259, 260:
    between bf16 values (spacing 2 from 256 on), both kinds of tie included (257 -> 256, 259 -> 260)"""
    return (248 + torch.arange(Cf) % 4).float().repeat(TOTAL, 1).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------
# the dense convolution the sparse backward replaces (for the CPU pin)
# ------------------------------------------------------------------------------------------------
def y_from_weights(g_t: torch.Tensor, Wt: torch.Tensor) -> torch.Tensor:
    """Y[s][tap][ci] = sum_co g_t[s][co] W[co][ci][tap / 3][tap % 3]: the contribution of the hidden-map gradient at an active pixel to
    the 3 x 3 neighbourhood of the level feature"""
    Co, Ci = Wt.shape[:2]
    return torch.einsum("so,oit->sti", g_t.double(), Wt.double().reshape(Co, Ci, 9))


def autograd_delta(rows: Sequence[int], g_t: torch.Tensor, Wt: torch.Tensor) -> torch.Tensor:
    """d(sum(conv2d(feat, W, padding=1) * gout))/d(feat) per level in fp64, gout zero off the active pixels; [TOTAL, Ci]"""
    Co, Ci = Wt.shape[:2]
    out = torch.zeros(TOTAL, Ci, dtype=torch.float64)
    for l, (H, W) in enumerate(LEVELS):
        feat = torch.zeros(N, Ci, H, W, dtype=torch.float64, requires_grad=True)
        gout = torch.zeros(N, Co, H, W, dtype=torch.float64)
        for s, row in enumerate(rows):
            ll, n, h, w = pixel_of(row)
            if ll == l:
                gout[n, :, h, w] = g_t[s].double()
        y = torch.nn.functional.conv2d(feat, Wt.double(), padding=1)
        (gf,) = torch.autograd.grad(y, feat, gout)
        out[ROW0[l]:ROW0[l + 1]] = gf.permute(0, 2, 3, 1).reshape(-1, Ci)
    return out

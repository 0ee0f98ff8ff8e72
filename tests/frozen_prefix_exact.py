"""Operands and CPU references for the exact-arithmetic tests of the frozen prefix (stem, stem + pool, max-pool, the res2 bottlenecks).

The operands are built so that the answer does not depend on the order of a sum or on where a rounding falls, which lets a kernel be
held to torch.equal:

  integer lattice    small integers everywhere: every partial sum is an integer far below 2^24 (exact in fp32 in any order), every value
                     that is rounded to bf16 is an integer of magnitude <= 256 (exact in bf16).  A dropped, doubled or misplaced term
                     changes an integer.
  single-term sums   one non-zero weight per output channel: a dot product is one bf16 x bf16 product (exact in fp32) plus exact zeros.
                     The operands are arbitrary reals, so every rounding of the epilogues is exercised; the references reproduce them
                     one rounding per operation.

The references are plain torch on the CPU: sums in fp64 (exact for both constructions), epilogues in the precision asked for.  Nothing
here touches the library under test.  Shared by test_frozen_prefix_exact_cpu.py and test_frozen_prefix_exact_gpu.py."""
import functools

import torch
import torch.nn.functional as F

PIXEL_MEAN, PIXEL_STD = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)

# the bottleneck tile is 8 x 16 pixels with a 10 x 18 halo: every halo pixel outside the image | exactly one tile | tail tiles one pixel
# wide and high | seams between images (the halo row below image n is in-range memory of image n + 1) | 3 x 3 tiles per image, 18 in all
BNECK_SHAPES = [(1, 1, 1), (1, 8, 16), (1, 9, 17), (3, 21, 19), (2, 17, 33)]
BNECK_FORMS = {"cin64": (64, False), "cin256": (256, False), "shortcut": (64, True)}      # name -> (Cin, projection shortcut in the kernel)
# one image of one pixel | smaller than one pooled tile | one pixel past a padding boundary | a ragged batch
STEM_SIZES = [[(1, 1)], [(9, 11)], [(33, 65)], [(61, 93), (37, 50), (64, 96)]]
STEM_SETS = ["single0", "single1", "single2", "lattice"]
TIE_CHANNELS = (4, 13, 40)          # all 4 mod 9: their only w2 tap is the centre one, so a tie pixel's a1 reaches the output pixel itself
TIE_LO, TIE_HI = 1.0, 1.0 + 2.0 ** -7
# the shortcut's two roundings fl(fl(acc * scale) + shift) against one fused multiply-add, in channel FMA_CHANNEL of the shortcut form:
# acc = 1 + 2^-7 and this fp32 scale give acc * scale = 1 + d with 2^-25 < d < 2^-24, so fl(acc * scale) = 1 and the sum with FMA_SHIFT
# is 0.5 + 2^-9 exactly, a bf16 tie that goes down to 0.5; fused, the sum keeps d, rounds to 0.5 + 2^-9 + 2^-24 and goes up to 0.5 + 2^-8
FMA_CHANNEL, FMA_SCALE, FMA_SHIFT = 22, 0.9922481179237366, -(0.5 - 2.0 ** -9)


# ------------------------------------------------------------------------------------------------ roundings
def bf16_rne(t):
    """round to nearest even onto the bf16 grid, in t's dtype (t fp32, or fp64 holding values the fp32 step does not move)"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    """the WRONG rounding: drop the low 16 bits"""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def fold(w, s):
    """what aldi_fold_weights_batch documents: bf16(w * scale[row]), the product in fp32"""
    return (w * s.view(-1, 1, 1, 1)).to(torch.bfloat16)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _ternary(shape, density, g):
    keep = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (keep * sign).float()


def _choice(values, n, g):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def _ints(lo, hi, shape, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ bottleneck operands
def bneck_seed(form, shape):
    Cin, sc = BNECK_FORMS[form]
    N, H, W = shape
    return 1000 * H + 10 * W + N + Cin + (7 if sc else 0)


def lattice_bneck(N, H, W, Cin, seed, shortcut=False):
    """ternary x (density 8 / Cin), w1 (1/4), w2 (1/16), w3 (1/8); scales {-1, 1, 2} / {-1, 1} / {-1, 1}; integer shifts in [-2, 2],
    [-3, 3], [-4, 4]; residual integers in [-8, 8].  At density 1/16 some (tap, input channel) columns of w2 come out empty (about nine
    of the 576): each gets one +-1 at a random output channel, so that every tap and every k-step of every tap contributes."""
    g = torch.Generator().manual_seed(seed)
    op = dict(N=N, H=H, W=W, Cin=Cin, kind="lattice")
    op["x"] = _ternary((N, H, W, Cin), 8.0 / Cin, g).to(torch.bfloat16)
    w1, w2, w3 = _ternary((64, 1, 1, Cin), 1 / 4, g), _ternary((64, 3, 3, 64), 1 / 16, g), _ternary((256, 1, 1, 64), 1 / 8, g)
    empty = (w2 != 0).sum(0) == 0
    for kh, kw, ci in empty.nonzero().tolist():
        w2[int(torch.randint(0, 64, (1,), generator=g)), kh, kw, ci] = float(torch.randint(0, 2, (1,), generator=g)) * 2 - 1
    op["w"] = [w1, w2, w3]
    op["s"] = [_choice([-1, 1, 2], 64, g), _choice([-1, 1], 64, g), _choice([-1, 1], 256, g)]
    op["b"] = [_ints(-2, 2, (64,), g), _ints(-3, 3, (64,), g), _ints(-4, 4, (256,), g)]
    op["res"] = _ints(-8, 8, (N, H, W, 256), g).to(torch.bfloat16)
    if shortcut:
        op["wsc"] = _ternary((256, 1, 1, 64), 1 / 8, g).to(torch.bfloat16)
        op["ssc"], op["bsc"] = _choice([-1, 1], 256, g), _ints(-4, 4, (256,), g)
    return op


def tie_pixels(N, H, W):
    return sorted({(0, 0, 0), (N - 1, H - 1, W - 1), (0, H // 2, W // 2)})


def single_term_bneck(N, H, W, Cin, seed, shortcut=False):
    """real-valued bf16 x and residual, real scales in [0.5, 1.5] and shifts; the folded weight of output row co has ONE non-zero: w1 at
    input channel co mod Cin, w2 at (input channel co, tap co mod 9), w3 and wsc at mid channel co mod 64.
    Rounding ties in TIE_CHANNELS at tie_pixels(): folded weights 1, b1 = 2^-8, b2 = b3 = 0, residual 0, x = 1 (channel 4) or 1 + 2^-7
    (13, 40), so the output there is bf16(x + 2^-8): 1 and 1 + 2^-6 to nearest even; 1 and 1 + 2^-7 truncated.
    Shortcut form: channel FMA_CHANNEL tells the two roundings of the shortcut's epilogue from a fused multiply-add (see FMA_SCALE): its
    conv3 sum is 0 (b2 = -100 empties mid channel 22, b3 = 0), so the output at the tie pixels is the shortcut itself, 0.5."""
    g = torch.Generator().manual_seed(seed)
    op = dict(N=N, H=H, W=W, Cin=Cin, kind="single")

    def vals(n):
        return (0.5 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)

    x = torch.randn(N, H, W, Cin, generator=g).to(torch.bfloat16)
    res = torch.randn(N, H, W, 256, generator=g).to(torch.bfloat16)
    w1, w2, w3 = torch.zeros(64, 1, 1, Cin), torch.zeros(64, 3, 3, 64), torch.zeros(256, 1, 1, 64)
    v1, v2, v3 = vals(64), vals(64), vals(256)
    co = torch.arange(64)
    w1[co, 0, 0, co % Cin] = v1
    w2[co, (co % 9) // 3, (co % 9) % 3, co] = v2
    co3 = torch.arange(256)
    w3[co3, 0, 0, co3 % 64] = v3
    s = [0.5 + torch.rand(c, generator=g) for c in (64, 64, 256)]
    b = [torch.randn(c, generator=g) * 0.3 for c in (64, 64, 256)]
    if shortcut:
        wsc = torch.zeros(256, 1, 1, 64)
        wsc[co3, 0, 0, co3 % 64] = vals(256)
        ssc, bsc = 0.5 + torch.rand(256, generator=g), torch.randn(256, generator=g) * 0.3
    for c in TIE_CHANNELS:
        assert c % 9 == 4 and c < 64
        w1[c, 0, 0, c], w2[c, 1, 1, c], w3[c, 0, 0, c] = 1.0, 1.0, 1.0
        s[0][c], s[1][c], s[2][c] = 1.0, 1.0, 1.0
        b[0][c], b[1][c], b[2][c] = 2.0 ** -8, 0.0, 0.0
        if shortcut:
            wsc[c], bsc[c] = 0.0, 0.0
        for n, h, w_ in tie_pixels(N, H, W):
            x[n, h, w_, c] = TIE_LO if c == TIE_CHANNELS[0] else TIE_HI
            res[n, h, w_, c] = 0.0
    if shortcut:
        c = FMA_CHANNEL
        wsc[c, 0, 0, c], ssc[c], bsc[c] = 1.0, FMA_SCALE, FMA_SHIFT
        b[1][c], b[2][c] = -100.0, 0.0
        for n, h, w_ in tie_pixels(N, H, W):
            x[n, h, w_, c] = TIE_HI
    op.update(x=x, res=res, w=[w1, w2, w3], s=s, b=b)
    if shortcut:
        op.update(wsc=wsc.to(torch.bfloat16), ssc=ssc, bsc=bsc)
    return op


# ------------------------------------------------------------------------------------------------ bottleneck reference
def _exact(acc, ep):
    """an fp64 sum in the epilogue's precision; both constructions make it exactly representable there"""
    out = acc.to(ep)
    assert torch.equal(out.double(), acc), "the operands do not keep their promise: a dot product is not exact in the epilogue's precision"
    return out


def bneck_reference(op, *, ep=torch.float64, rnd=bf16_rne, halo="zero", drop_tap=None, sc_fma=False, maps=None):
    """y = relu( bf16(W3 a2 + b3) + r ),  a2 = bf16(relu(W2 (*) a1 + b2)),  a1 = bf16(relu(W1 x + b1)), a1 zero outside the image;
    r = the residual, or with op["wsc"] the projection shortcut bf16((Wsc x) * scale + shift).  Weights folded as fold() does.  Sums in
    fp64, epilogues in `ep`, one rounding per operation.  Returns bf16 [N, H, W, 256].  `maps` (a dict) receives every value BEFORE it is
    rounded to bf16.  The deliberately WRONG forms (for the tests that show the operands can tell them apart):
      halo = "relu_b1"     conv1 is evaluated on zero-padded x, so the out-of-image halo of a1 holds relu(b1)
      halo = "next_image"  the halo row below image n is row 0 of image n + 1 (what the flat NHWC address of that row holds)
      drop_tap = (kh, kw)  that tap of w2 contributes nothing
      rnd = bf16_trunc     truncation in place of round to nearest even
      sc_fma = True        the shortcut's acc * scale + shift with ONE rounding (a fused multiply-add)"""
    N = op["N"]
    f1, f2, f3 = [_nchw(fold(w, s).double()) for w, s in zip(op["w"], op["s"])]
    b1, b2, b3 = [b.to(ep).view(1, -1, 1, 1) for b in op["b"]]
    if drop_tap is not None:
        f2 = f2.clone()
        f2[:, :, drop_tap[0], drop_tap[1]] = 0
    x = _nchw(op["x"].double())
    rec = maps if maps is not None else {}
    if halo == "relu_b1":
        rec["p1"] = _exact(F.conv2d(F.pad(x, (1, 1, 1, 1)), f1), ep) + b1
        a1p = rnd(F.relu(rec["p1"]))
    else:
        rec["p1"] = _exact(F.conv2d(x, f1), ep) + b1
        a1 = rnd(F.relu(rec["p1"]))
        a1p = F.pad(a1, (1, 1, 1, 1))
        if halo == "next_image":
            a1p[:N - 1, :, -1, 1:-1] = a1[1:, :, 0, :]
        else:
            assert halo == "zero", halo
    rec["p2"] = _exact(F.conv2d(a1p.double(), f2), ep) + b2
    a2 = rnd(F.relu(rec["p2"]))
    rec["p3"] = _exact(F.conv2d(a2.double(), f3), ep) + b3
    s3 = rnd(rec["p3"])
    if "wsc" in op:
        acc = _exact(F.conv2d(x, _nchw(op["wsc"].double())), ep)
        rec["psc"] = acc * op["ssc"].to(ep).view(1, -1, 1, 1) + op["bsc"].to(ep).view(1, -1, 1, 1)       # two operations, two roundings
        if sc_fma:
            rec["psc"] = (acc.double() * op["ssc"].double().view(1, -1, 1, 1) + op["bsc"].double().view(1, -1, 1, 1)).to(ep)
        r = rnd(rec["psc"])
    else:
        r = _nchw(op["res"]).to(ep)
    rec["p4"] = s3 + r
    y = rnd(F.relu(rec["p4"]))
    return y.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def bneck_case(kind, form, shape):
    """(operands, reference output) of one GPU case, computed once per session; treat both as read-only"""
    Cin, sc = BNECK_FORMS[form]
    seed = bneck_seed(form, shape)
    if kind == "lattice":
        op = lattice_bneck(*shape, Cin, seed, sc)
        return op, bneck_reference(op, ep=torch.float64)
    op = single_term_bneck(*shape, Cin, seed, sc)
    return op, bneck_reference(op, ep=torch.float32)


# ------------------------------------------------------------------------------------------------ stem operands
def stage_images(sizes, seed, lattice):
    """uint8 [N, 3, Hs, Ws]: image n in the top-left h x w, zeros elsewhere, Hs / Ws the batch maximum padded to a multiple of 32"""
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = (max(s[0] for s in sizes) + 31) // 32 * 32, (max(s[1] for s in sizes) + 31) // 32 * 32
    img = torch.zeros(len(sizes), 3, Hs, Ws, dtype=torch.uint8)
    for i, (h, w) in enumerate(sizes):
        img[i, :, :h, :w] = torch.randint(0, 2 if lattice else 256, (3, h, w), generator=g, dtype=torch.uint8)
    return img


def stem_single_term(k, seed):
    """weight set k of three: channel co has its only non-zero at flat tap 49 k + co of the 147 taps (kh, kw, c), none where that exceeds
    146; bf16-exact real values; real scale and shift; the project's pixel mean and std"""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(64, 147)
    v = ((0.25 + torch.rand(64, generator=g)) * (torch.randint(0, 2, (64,), generator=g) * 2 - 1)).to(torch.bfloat16).float()
    for co in range(64):
        if 49 * k + co < 147:
            w[co, 49 * k + co] = v[co]
    return dict(w=w.view(64, 7, 7, 3), scale=0.5 + torch.rand(64, generator=g), shift=torch.randn(64, generator=g) * 0.3,
                mean=PIXEL_MEAN, std=PIXEL_STD, kind="single")


def stem_lattice(seed):
    """image in {0, 1} (stage_images(lattice=True)), mean 0, std 1, dense ternary weights (density 1/2), scale in {-1, 1, 2}, integer shift"""
    g = torch.Generator().manual_seed(seed)
    return dict(w=_ternary((64, 7, 7, 3), 1 / 2, g), scale=_choice([-1, 1, 2], 64, g), shift=_ints(-3, 3, (64,), g),
                mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), kind="lattice")


def stem_reference(img, sizes, ws, dtype, *, pad_normalised=False, maps=None):
    """(conv [N, Hs/2, Ws/2, 64], pooled [N, Hs/4, Ws/4, 64]) in `dtype`, every step in fp32 with one rounding per operation:
        v = (float(px) - mean) * (1.0f / std), zero outside the image (the conv pads the NORMALISED image); bf16 path: v to bf16
        acc = sum of v * w over the 7 x 7 x 3 window, stride 2, pad 3 (fp64, then one rounding to fp32: the single product, or an integer)
        t = relu(fl(fl(acc * scale) + shift)) rounded to dtype;  pooled = 3 x 3 stride 2 pad 1 maximum over in-range conv outputs
    pad_normalised = True is the WRONG form in which the pad region holds (0 - mean) / std."""
    mean = torch.tensor(ws["mean"], dtype=torch.float32).view(1, 3, 1, 1)
    inv = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(ws["std"], dtype=torch.float32)).view(1, 3, 1, 1)
    v = (img.float() - mean) * inv
    if not pad_normalised:
        inside = torch.zeros_like(v, dtype=torch.bool)
        for i, (h, w) in enumerate(sizes):
            inside[i, :, :h, :w] = True
        v = torch.where(inside, v, torch.zeros_like(v))
    wt = ws["w"]
    if dtype == torch.bfloat16:
        v, wt = v.to(torch.bfloat16).float(), wt.to(torch.bfloat16).float()
    acc = F.conv2d(v.double(), _nchw(wt).double(), stride=2, padding=3).float()
    t = acc * ws["scale"].view(1, -1, 1, 1) + ws["shift"].view(1, -1, 1, 1)
    if maps is not None:
        maps["acc"], maps["t"] = acc, t
    y = F.relu(t).to(dtype)
    pooled = F.max_pool2d(y.float(), kernel_size=3, stride=2, padding=1).to(dtype)
    return y.permute(0, 2, 3, 1).contiguous(), pooled.permute(0, 2, 3, 1).contiguous()


def stem_weights(name):
    return stem_lattice(77) if name == "lattice" else stem_single_term(int(name[-1]), 31 + int(name[-1]))


@functools.lru_cache(maxsize=None)
def stem_case(name, size_idx):
    """(image, sizes, weight set, {dtype: (conv, pooled)}) of one GPU case, computed once per session; read-only"""
    sizes = STEM_SIZES[size_idx]
    ws = stem_weights(name)
    img = stage_images(sizes, 100 + size_idx, ws["kind"] == "lattice")
    return img, sizes, ws, {dt: stem_reference(img, sizes, ws, dt) for dt in (torch.float32, torch.bfloat16)}


# ------------------------------------------------------------------------------------------------ reporting
def mismatch_report(got, want, what, limit=8):
    """'' if got == want everywhere (NaN never equals), else the count of differing elements and the (n, h, w, c) of the first few"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return ""
    bad = (got.float() != want.float()) | got.float().isnan()
    idx = bad.nonzero()
    lines = [f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first (n, h, w, c): got / want"]
    for n, h, w, c in idx[:limit].tolist():
        lines.append(f"  ({n}, {h}, {w}, {c}): {float(got[n, h, w, c])!r} / {float(want[n, h, w, c])!r}")
    return "\n".join(lines)

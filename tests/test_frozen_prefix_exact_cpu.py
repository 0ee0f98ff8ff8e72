"""The operands and references of test_frozen_prefix_exact_gpu.py, checked without a GPU: the lattice operands keep the promise that makes
torch.equal a fair demand; deliberately wrong references differ from the true one exactly where the error they model lives (so a kernel
with that error cannot pass); and the references agree with the oracle's conv_bn / relu / max_pool2d."""
import pytest
import torch
import torch.nn.functional as F

import frozen_prefix_exact as X
from oracle import d2_rcnn as R

BNECK_CASES = [(f, s) for f in X.BNECK_FORMS for s in X.BNECK_SHAPES]
U = 2.0 ** -24          # fp32 unit roundoff


def _ids(cases):
    return ["-".join(str(v).replace(" ", "") for v in c) for c in cases]


# ------------------------------------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_bottleneck_lattice_preconditions(form, shape):
    """conditions on the inputs of every lattice case the GPU test runs (a seed that violates one is replaced, the condition stays)"""
    Cin, sc = X.BNECK_FORMS[form]
    op = X.lattice_bneck(*shape, Cin, X.bneck_seed(form, shape), sc)
    maps = {}
    y = X.bneck_reference(op, ep=torch.float64, maps=maps)
    assert set(maps) == ({"p1", "p2", "p3", "p4", "psc"} if sc else {"p1", "p2", "p3", "p4"})
    for k, m in maps.items():
        assert m.dtype == torch.float64
        assert torch.equal(X.bf16_rne(m), m), f"{k}: a value that gets rounded is not exact in bf16"
        assert float(m.abs().max()) <= 256, (k, float(m.abs().max()))
        assert torch.equal(m, m.round()), k
    pos = float((y.float() > 0).float().mean())
    assert 0.2 <= pos <= 0.8, pos
    assert int((op["b"][0] > 0).sum()) > 0, "b1 needs positive entries: relu(b1) in the halo must be visible"
    w1, w2, w3 = op["w"]
    assert bool(((w2 != 0).sum(0) > 0).all()), "every (tap, input channel) of w2 feeds some output channel"
    assert bool(((w1 != 0).sum(0) > 0).all()) and bool(((w3 != 0).sum(0) > 0).all())
    for w, s in zip(op["w"], op["s"]):
        assert torch.equal(X.fold(w, s).float(), w * s.view(-1, 1, 1, 1)), "folded weights are exact"


@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_bottleneck_single_term_operands(form, shape):
    Cin, sc = X.BNECK_FORMS[form]
    op = X.single_term_bneck(*shape, Cin, X.bneck_seed(form, shape), sc)
    for w, s in zip(op["w"], op["s"]):
        f = X.fold(w, s).float().flatten(1)
        assert bool(((f != 0).sum(1) == 1).all()), "one non-zero per row of every folded weight"
    w2 = X.fold(op["w"][1], op["s"][1]).float()
    assert bool(((w2 != 0).sum((0, 3)) > 0).all()), "one launch covers all nine taps"
    y = X.bneck_reference(op, ep=torch.float32).float()
    if y.numel() >= 256 * 128:
        assert 0.2 <= float((y > 0).float().mean()) <= 0.8
    # the planted ties: bf16(1 + 2^-8) = 1 and bf16(1 + 2^-7 + 2^-8) = 1 + 2^-6 to nearest even
    for n, h, w_ in X.tie_pixels(*shape):
        for c in X.TIE_CHANNELS:
            assert float(y[n, h, w_, c]) == (1.0 if c == X.TIE_CHANNELS[0] else 1.0 + 2.0 ** -6), (n, h, w_, c, float(y[n, h, w_, c]))


@pytest.mark.parametrize("size_idx", range(len(X.STEM_SIZES)))
def test_stem_lattice_preconditions(size_idx):
    img, sizes, ws, refs = X.stem_case("lattice", size_idx)
    for dt in (torch.float32, torch.bfloat16):
        maps = {}
        y, pooled = X.stem_reference(img, sizes, ws, dt, maps=maps)
        for k, m in maps.items():
            assert torch.equal(m, m.round()) and torch.equal(X.bf16_rne(m), m) and float(m.abs().max()) <= 256, k
        assert 0.2 <= float((y.float() > 0).float().mean()) <= 0.8
        assert torch.equal(y, refs[dt][0]) and torch.equal(pooled, refs[dt][1])
    assert torch.equal(refs[torch.float32][0], refs[torch.bfloat16][0].float()), "on the lattice both precisions give the same integers"


def test_stem_single_term_sets_cover_every_tap():
    hit = torch.zeros(147, dtype=torch.bool)
    for k in range(3):
        w = X.stem_single_term(k, 31 + k)["w"].reshape(64, 147)
        assert int(((w != 0).sum(1) > 1).sum()) == 0, "at most one non-zero per channel"
        assert torch.equal(w.to(torch.bfloat16).float(), w), "bf16-exact weight values"
        for co in range(64):
            nz = (w[co] != 0).nonzero().flatten().tolist()
            assert nz == ([49 * k + co] if 49 * k + co < 147 else []), (k, co, nz)
        hit |= (w != 0).any(0)
    assert bool(hit.all())
    wl = X.stem_lattice(77)["w"].reshape(64, 147)
    assert bool((wl != 0).any(0).all())


# ------------------------------------------------------------------------------------------------ the inputs discriminate
def _pixel_diff(a, b):
    return (a.float() != b.float()).any(-1)          # [N, H, W]


@pytest.mark.parametrize("kind", ["lattice", "single"])
@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_relu_b1_in_the_halo_shows_at_the_border_only(kind, form, shape):
    """the classic error of a fused bottleneck: conv1 evaluated on the zero-padded x, relu(b1) where conv2 must see zero padding"""
    op, want = X.bneck_case(kind, form, shape)
    ep = torch.float64 if kind == "lattice" else torch.float32
    wrong = X.bneck_reference(op, ep=ep, halo="relu_b1")
    N, H, W = shape
    border = torch.zeros(N, H, W, dtype=torch.bool)
    border[:, 0], border[:, -1], border[:, :, 0], border[:, :, -1] = True, True, True, True
    d = _pixel_diff(wrong, want)
    assert int((d & ~border).sum()) == 0
    assert int(d.sum()) > 0.9 * int(border.sum()), (int(d.sum()), int(border.sum()))


@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_dropped_w2_tap_shows(form, shape):
    op, want = X.bneck_case("lattice", form, shape)
    N, H, W = shape
    for kh in range(3):
        for kw in range(3):
            wrong = X.bneck_reference(op, ep=torch.float64, drop_tap=(kh, kw))
            reaches = (H > 1 or kh == 1) and (W > 1 or kw == 1)          # (a one-pixel image only ever sees the centre tap)
            assert bool(_pixel_diff(wrong, want).any()) == reaches, (kh, kw)


@pytest.mark.parametrize("kind", ["lattice", "single"])
@pytest.mark.parametrize("form,shape", [c for c in BNECK_CASES if c[1][0] > 1], ids=_ids([c for c in BNECK_CASES if c[1][0] > 1]))
def test_halo_from_the_next_image_shows_at_the_seam_rows(kind, form, shape):
    op, want = X.bneck_case(kind, form, shape)
    wrong = X.bneck_reference(op, ep=torch.float64 if kind == "lattice" else torch.float32, halo="next_image")
    N, H, W = shape
    seam = torch.zeros(N, H, W, dtype=torch.bool)
    seam[:N - 1, H - 1] = True
    d = _pixel_diff(wrong, want)
    assert int((d & ~seam).sum()) == 0
    assert int(d.sum()) > 0.9 * int(seam.sum()), (int(d.sum()), int(seam.sum()))


@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_truncation_shows_at_the_planted_ties(form, shape):
    op, want = X.bneck_case("single", form, shape)
    wrong = X.bneck_reference(op, ep=torch.float32, rnd=X.bf16_trunc).float()
    for n, h, w_ in X.tie_pixels(*shape):
        lo, *hi = X.TIE_CHANNELS
        assert float(wrong[n, h, w_, lo]) == float(want[n, h, w_, lo]) == 1.0           # 1 + 2^-8: the tie goes DOWN to the even neighbour
        for c in hi:                                                                     # 1 + 2^-7 + 2^-8: the tie goes UP, truncation down
            assert float(wrong[n, h, w_, c]) == 1.0 + 2.0 ** -7 and float(want[n, h, w_, c]) == 1.0 + 2.0 ** -6, (n, h, w_, c)


@pytest.mark.parametrize("shape", X.BNECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_multiply_add_in_the_shortcut_shows_at_the_planted_pixels(shape):
    from fractions import Fraction
    scale = Fraction(float(torch.tensor(X.FMA_SCALE, dtype=torch.float32)))
    d = Fraction(X.TIE_HI) * scale - 1
    assert Fraction(1, 2 ** 25) < d < Fraction(1, 2 ** 24), "fl(acc * scale) = 1, and the fused sum stays above the bf16 tie"
    op, want = X.bneck_case("single", "shortcut", shape)
    wrong = X.bneck_reference(op, ep=torch.float32, sc_fma=True)
    for n, h, w_ in X.tie_pixels(*shape):
        assert float(want[n, h, w_, X.FMA_CHANNEL]) == 0.5 and float(wrong[n, h, w_, X.FMA_CHANNEL]) == 0.5 + 2.0 ** -8, (n, h, w_)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size_idx", range(len(X.STEM_SIZES)))
def test_unnormalised_zero_in_the_stem_pad_shows_at_the_image_edges(size_idx, dtype):
    """a pad region that holds (0 - mean) / std: inside an image's own conv outputs only those whose 7 x 7 window (pad 3) reaches past
    the right or bottom edge may change -- within three input pixels of it -- and an image that fills the staging buffer not at all"""
    seen = False
    for name in ("single0", "single1", "single2"):
        img, sizes, ws, refs = X.stem_case(name, size_idx)
        wrong, _ = X.stem_reference(img, sizes, ws, dtype, pad_normalised=True)
        d = _pixel_diff(wrong, refs[dtype][0])
        Hs, Ws = img.shape[2:]
        for i, (h, w) in enumerate(sizes):
            own = d[i, :(h + 1) // 2, :(w + 1) // 2]
            oy = torch.arange(own.shape[0]).view(-1, 1) * 2 + 3
            ox = torch.arange(own.shape[1]).view(1, -1) * 2 + 3
            near = ((oy >= h) & (h < Hs)) | ((ox >= w) & (w < Ws))
            assert int((own & ~near).sum()) == 0, (name, i)
            if (h, w) == (Hs, Ws):
                assert not bool(d[i].any())
            seen |= bool((own & near).any())
    assert seen


# ------------------------------------------------------------------------------------------------ tie to the oracle
def _sd(prefix, w_nhwc, scale, shift, sd=None):
    """a FrozenBN whose folded scale and shift are the intended ones: weight = scale, bias = shift, mean 0, var = 1 - eps"""
    sd = {} if sd is None else sd
    sd[prefix + ".weight"] = w_nhwc.float().permute(0, 3, 1, 2).contiguous()
    sd[prefix + ".norm.weight"], sd[prefix + ".norm.bias"] = scale.clone(), shift.clone()
    sd[prefix + ".norm.running_mean"] = torch.zeros_like(scale)
    sd[prefix + ".norm.running_var"] = torch.full_like(scale, 1.0 - R.BN_EPS)
    return sd


def _stage_bound(e_in, a_abs, w_nhwc, scale, shift, stride=1, pad=0):
    """how far the oracle's fp32 conv_bn may land from the exact value when its input is within e_in of the exact input a.
    The oracle's scale is fl(s * fl(rsqrt(fl(fl(1 - eps) + eps)))) = s (1 + t), |t| <= 4 U: one rounding each for storing the variance,
    adding eps (each moves rsqrt by half as much), rsqrt itself (2 U) and the product.  A K-term fp32 dot product is within K U of its
    exact value, relative to the sum of magnitudes -- and exact when its input is (e_in = 0: integers, every partial sum far below
    2^24); the scale, the multiply and the add bring 6 U more.  So, to first order in U,
        e_out <= A e_in + (K + 6) U (T + A e_in),   T = max(|s| . (|w| (*) |a|) + |shift|),   A = max over rows of |s| . sum |w|"""
    wa = w_nhwc.double().abs().permute(0, 3, 1, 2)
    K = wa[0].numel() if e_in > 0 else 0
    T = float((F.conv2d(a_abs.double(), wa, stride=stride, padding=pad) * scale.double().abs().view(1, -1, 1, 1)
               + shift.double().abs().view(1, -1, 1, 1)).max())
    A = float((wa.flatten(1).sum(1) * scale.double().abs()).max())
    return A * e_in + (K + 6) * U * (T + A * e_in)


@pytest.mark.parametrize("form,shape", BNECK_CASES, ids=_ids(BNECK_CASES))
def test_bottleneck_reference_agrees_with_the_oracle(form, shape):
    op, want = X.bneck_case("lattice", form, shape)
    sd = {}
    for k, (w, s, b) in enumerate(zip(op["w"], op["s"], op["b"])):
        _sd(f"c{k + 1}", w, s, b, sd)
    x = op["x"].float().permute(0, 3, 1, 2)
    a1 = F.relu(R.conv_bn(x, sd, "c1"))
    a2 = F.relu(R.conv_bn(a1, sd, "c2", 1, 1))
    h = R.conv_bn(a2, sd, "c3")
    # the bound, stage by stage, from the exact maps of the reference (integers: the bf16 roundings between the stages move nothing)
    maps = {}
    X.bneck_reference(op, ep=torch.float64, maps=maps)
    e = _stage_bound(0.0, x.abs(), op["w"][0], op["s"][0], op["b"][0])
    e = _stage_bound(e, F.relu(maps["p1"]), op["w"][1], op["s"][1], op["b"][1], pad=1)
    e = _stage_bound(e, F.relu(maps["p2"]), op["w"][2], op["s"][2], op["b"][2])
    if "wsc" in op:
        _sd("sc", op["wsc"], op["ssc"], op["bsc"], sd)
        r = R.conv_bn(x, sd, "sc")
        e += _stage_bound(0.0, x.abs(), op["wsc"], op["ssc"], op["bsc"])
    else:
        r = op["res"].float().permute(0, 3, 1, 2)
    e += U * float(maps["p4"].abs().max())
    got = F.relu(h + r).permute(0, 2, 3, 1)
    assert e < 0.25, e          # below half the lattice spacing: within the bound, the oracle rounds to the very integers of the reference
    err = float((got.double() - want.double()).abs().max())
    assert err <= e, (err, e)


@pytest.mark.parametrize("size_idx", range(len(X.STEM_SIZES)))
def test_stem_reference_agrees_with_the_oracle(size_idx):
    img, sizes, ws, refs = X.stem_case("lattice", size_idx)
    sd = _sd("stem", ws["w"], ws["scale"], ws["shift"])
    cfg = R.make_cfg(pixel_mean=list(ws["mean"]), pixel_std=list(ws["std"]), size_divisibility=32)
    x, got_sizes = R.preprocess(cfg, [img[i, :, :h, :w] for i, (h, w) in enumerate(sizes)])
    assert got_sizes == [tuple(s) for s in sizes] and x.shape == img.shape
    y = F.relu(R.conv_bn(x, sd, "stem", 2, 3))
    pooled = F.max_pool2d(y, kernel_size=3, stride=2, padding=1)
    e = _stage_bound(0.0, x.abs(), ws["w"], ws["scale"], ws["shift"], stride=2, pad=3)
    assert e < 0.25, e
    want_y, want_p = refs[torch.float32]
    assert float((y.permute(0, 2, 3, 1) - want_y).abs().max()) <= e
    assert float((pooled.permute(0, 2, 3, 1) - want_p).abs().max()) <= e          # (max and relu are 1-Lipschitz)

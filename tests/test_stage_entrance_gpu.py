"""The entrance of a trainable stage (res3.0 / res4.0 / res5.0) in the bf16 trunk: the projection shortcut formed inside conv3's launch (the
"pair" form of the 1x1 igemm, csrc/igemm_pair.h), the stage-input gradient as one pair launch on the compact grid, and the zero-stuffed stride-2
residual (res_mode 3) that hands it to the lateral data gradient.  Everything here is bit for bit against the launches it replaces."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _default_knobs():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


# ---------------------------------------------------------------------------------------------------- the pair kernel against two launches
def _pair_operands(N, H, W, stride, Cin2, K, Cout, affine, shift_bias, seed):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bf = lambda t: t.to(torch.bfloat16).to(DEV).contiguous()
    x2 = bf(torch.randn(N, H, W, Cin2, generator=g))
    x = bf(torch.randn(N, Ho, Wo, K, generator=g))
    w2 = bf(torch.randn(Cout, 1, 1, Cin2, generator=g) / Cin2 ** 0.5)
    w = bf(torch.randn(Cout, 1, 1, K, generator=g) / K ** 0.5)
    if not affine:
        return x2, x, w2, w, None, None, None, None
    s2, s = [(torch.rand(Cout, generator=g) + 0.5).to(DEV) for _ in range(2)]
    b2 = (torch.randn(Cout, generator=g) * 0.3 + shift_bias).to(DEV)
    b = (torch.randn(Cout, generator=g) * 0.3).to(DEV)
    return x2, x, w2, w, s2, b2, s, b


# (N, H, W of x2, stride, Cin2, K of the main conv, Cout, scale / shift / ReLU, bias of shift2)
PAIR_SHAPES = [
    (1, 16, 32, 2, 128, 64, 64, True, 0.0),          # exactly one 128 x 64 tile
    (3, 21, 19, 2, 256, 128, 192, True, 0.0),        # odd H and W; 330 rows: a ragged last tile, image boundaries inside tiles; three column tiles
    (2, 12, 16, 2, 1024, 512, 2048, True, 0.0),      # res5.0's channels at the engine tests' size: one partial tile, 32 inner slabs
    (3, 11, 10, 1, 256, 64, 128, False, 0.0),        # stride 1, no scale / shift / ReLU: the backward form
    (3, 21, 19, 2, 256, 128, 192, True, -2.0),       # the shortcut's shift pulls most sums under the ReLU
]


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("N,H,W,stride,Cin2,K,Cout,affine,shift_bias", PAIR_SHAPES)
def test_pair_equals_two_launches(N, H, W, stride, Cin2, K, Cout, affine, shift_bias, two):
    """reference forced onto the epilogue whose rounding the flag names: igemm_direct 0 = staged (two roundings), igemm_force 2 = direct (one);
    rounding 0 makes the pair launch derive the same flag from the same knobs"""
    from aldi_amd import _lib as L, ops
    x2, x, w2, w, s2, b2, s, b = _pair_operands(N, H, W, stride, Cin2, K, Cout, affine, shift_bias, 1000 * H + 10 * W + Cout)
    if two:
        L.set_tuning("igemm_direct", 0)
    else:
        L.set_tuning("igemm_force", 2)
    M = x.shape[0] * x.shape[1] * x.shape[2]
    bits_w, bits_g = [torch.zeros(M * Cout // 8, dtype=torch.uint8, device=DEV) for _ in range(2)]
    sc = ops.conv2d(x2, w2, stride=stride, scale=s2, shift=b2)
    want = ops.conv2d(x, w, scale=s, shift=b, res=sc, res_mode=1, relu=affine, bits_out=bits_w)
    ref_name = L.last_dispatch()
    assert ("direct+res" in ref_name) == (not two), ref_name
    got = ops.conv2d(x, w, scale=s, shift=b, relu=affine, bits_out=bits_g, pre=(x2, w2, s2, b2, stride))
    name = L.last_dispatch()
    torch.cuda.synchronize()
    assert name.startswith("igemm_pair<") and ("round2" if two else "round1") in name, name
    assert float(want.float().abs().max()) > 0
    if shift_bias:
        clipped = float((want == 0).float().mean())
        assert 0.02 < clipped < 0.98, clipped
    assert torch.equal(got, want)
    assert torch.equal(bits_g, bits_w)
    # the explicit flag gives the same launch whatever the knobs say
    L.reset_tuning()
    got2 = ops.conv2d(x, w, scale=s, shift=b, relu=affine, pre=(x2, w2, s2, b2, stride, 2 if two else 1))
    torch.cuda.synchronize()
    assert torch.equal(got2, want)


# ---------------------------------------------------------------------------------------------------- res_mode 3
@pytest.mark.parametrize("knob,value,expect", [("igemm_direct", 0, "staged"), ("igemm_force", 2, "igemm<bf16,128,64,4,1,pipe,tap,direct+res>"),
                                               ("igemm_force", 14, "igemm_ws<bf16,32,128,k256>")])
@pytest.mark.parametrize("N,Ho,Wo", [(1, 8, 16), (3, 21, 19)])
def test_zero_stuffed_residual_equals_residual_map_of_zeros(N, Ho, Wo, knob, value, expect):
    """res_mode 3 on the compact [N][(Ho+1)/2][(Wo+1)/2][C] map == res_mode 1 on the full-size map that is zero except at even (ho, wo), on
    each of the three kernels a lateral data gradient can land on (and mode 3 lands where mode 1 does)"""
    from aldi_amd import _lib as L, ops
    K, Cout = 256, 128
    g = torch.Generator().manual_seed(100 * Ho + Wo)
    x = torch.randn(N, Ho, Wo, K, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(Cout, 1, 1, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    small = torch.randn(N, (Ho + 1) // 2, (Wo + 1) // 2, Cout, generator=g).to(torch.bfloat16).to(DEV)
    bits = torch.randint(0, 256, (N * Ho * Wo * Cout // 8,), generator=g, dtype=torch.uint8).to(DEV)
    full = torch.zeros(N, Ho, Wo, Cout, dtype=torch.bfloat16, device=DEV)
    full[:, ::2, ::2] = small
    L.set_tuning(knob, value)
    want = ops.conv2d(x, w, res=full, res_mode=1, mask_bits=bits)
    name1 = L.last_dispatch()
    got = ops.conv2d(x, w, res=small, res_mode=3, mask_bits=bits)
    name3 = L.last_dispatch()
    torch.cuda.synchronize()
    assert name3 == name1, (name1, name3)
    if expect == "staged":
        assert name1.startswith("igemm<") and "direct" not in name1, name1
    else:
        assert name1 == expect, name1
    kept = float((want != 0).float().mean())
    assert 0.3 < kept < 0.7, kept                       # (random mask bits: about half of the outputs survive)
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def model():
    from aldi_amd import synthetic as syn
    from aldi_amd.arch import ParamLayout
    from aldi_amd.engine import RCNN, Weights
    K, H, W = 8, 192, 256
    w = Weights(ParamLayout(K), torch.device(DEV), torch.bfloat16, trainable=True)
    w.load_state_dict(syn.init_state_dict(K, seed=1))
    m = RCNN(w, K)
    assert m.knobs.fused_stage_entrance
    _, data, _, _ = syn.make_batch(2, 0, H, W, K, seed=0)
    st, sizes, _ = m.stage_images([d["image"] for d in data])
    return m, st, sizes


@pytest.mark.parametrize("save", [False, True])
def test_trunk_with_stage_entrance_fold_equals_trunk_without(model, save):
    """P2..P6 (and, saved for the backward, every block output's ReLU bits) with the three shortcuts inside their conv3 launches == with the
    shortcuts as launches of their own"""
    from aldi_amd import _lib as L
    m, st, sizes = model
    outs, bits, names = {}, {}, {}
    for fold in (True, False):
        seen = []
        conv = m.conv
        m.conv = lambda x, name, **kw: (conv(x, name, **kw), seen.append((name, L.last_dispatch())))[0]
        try:
            with m.with_knobs(fused_stage_entrance=fold):
                c = m.trunk(st, sizes, save=save)
        finally:
            del m.conv
        torch.cuda.synchronize()
        outs[fold], names[fold] = c.P, seen
        if save:
            bits[fold] = [c.out_bits[blk[4].data_ptr()] for blk in c.blocks]
    assert sum(n.endswith("shortcut") for n, _ in names[False]) == 3 and not any(n.endswith("shortcut") for n, _ in names[True])
    assert sum(d.startswith("igemm_pair<") for _, d in names[True]) == 3 and not any(d.startswith("igemm_pair<") for _, d in names[False])
    assert len(outs[True]) == 5 and float(outs[False][0].float().abs().max()) > 0
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
    if save:
        assert len(bits[True]) == 13
        for a, b in zip(bits[True], bits[False]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("si", [2, 3])
def test_stage_input_gradient_folded_equals_three_scattering_launches(model, si):
    """d(loss)/d(C4) (si = 3: res5's entrance) and d/d(C3) (si = 2) on random upstream gradients: pair launch + res_mode 3 == zero map, two
    scattering launches, full-size residual"""
    from aldi_amd import _lib as L
    from aldi_amd.engine import FPN_C, STAGE_BLOCKS
    m, st, sizes = model
    c = m.trunk(st, sizes, save=True)
    p, xin, h1, h2, out, first = c.blocks[sum(STAGE_BLOCKS[1:si])]
    assert first and p.endswith(f"res{si + 2}.0.") and c.out_bits.get(xin.data_ptr()) is not None
    gen = torch.Generator().manual_seed(si)
    rnd = lambda like, ch=None: torch.randn(*like.shape[:3], ch or like.shape[3], generator=gen).to(torch.bfloat16).to(DEV)
    g, g1, gprev = rnd(out), rnd(h1), rnd(xin, FPN_C)
    res = {}
    for fold in (True, False):
        with m.with_knobs(fused_stage_entrance=fold):
            res[fold] = m._stage_input_grad(c, si, p, xin, g, g1, gprev)
            res[fold, "name"] = L.last_dispatch()
            torch.cuda.synchronize()
    assert res[True, "name"] == res[False, "name"]        # the lateral's data gradient keeps its kernel
    assert res[True].shape == xin.shape and 0.05 < float((res[False] != 0).float().mean()) < 0.95
    assert torch.equal(res[True], res[False])

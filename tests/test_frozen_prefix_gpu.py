"""The frozen prefix of the bf16 trunk: the persistent stem + pool kernel against the two-kernel path, and the first res2 bottleneck with
its projection shortcut inside the kernel against the two-launch path.  Everything here is bit for bit: the fused forms keep the
per-element order of every sum and every rounding of the forms they replace."""
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


def _stem_both(sizes, seed):
    """(stem_pool_forward, maxpool3s2(stem_forward)) on random images of `sizes` in one zero-padded batch"""
    from aldi_amd import ops
    from aldi_amd.arch import pad_to
    gen = torch.Generator().manual_seed(seed)
    Hs, Ws = pad_to(max(s[0] for s in sizes), 32), pad_to(max(s[1] for s in sizes), 32)
    img = torch.zeros(len(sizes), 3, Hs, Ws, dtype=torch.uint8)
    for i, (h, w) in enumerate(sizes):
        img[i, :, :h, :w] = torch.randint(0, 256, (3, h, w), generator=gen, dtype=torch.uint8)
    w = (torch.randn(64, 7, 7, 3, generator=gen) * 0.05).to(DEV)
    scale = (0.5 + torch.rand(64, generator=gen)).to(DEV)
    shift = (torch.randn(64, generator=gen) * 0.3).to(DEV)
    mean, std = (103.53, 116.28, 123.675), (57.375, 57.12, 58.395)
    imgd = img.to(DEV)
    ref = ops.maxpool3s2(ops.stem_forward(imgd, sizes, w, scale, shift, mean, std, torch.bfloat16))
    got = ops.stem_pool_forward(imgd, sizes, ops.stem_pack_weights(w), scale, shift, mean, std)
    torch.cuda.synchronize()
    assert got.shape == ref.shape and float(ref.float().abs().max()) > 0
    return got, ref


# ragged batch; an image smaller than one pooled tile; more tiles than the persistent grid has workgroups and not a multiple of it
# (4 x 18 x 23 = 1656 tiles of 7 x 7 pooled pixels against two workgroups per compute unit)
@pytest.mark.parametrize("sizes", [[(61, 93), (37, 50), (64, 96)], [(9, 11)], [(480, 640)] * 4])
def test_persistent_stem_pool_equals_stem_then_maxpool(sizes):
    got, ref = _stem_both(sizes, 11 + len(sizes))
    assert torch.equal(got, ref)


@pytest.mark.parametrize("wgs", [1, 5])
def test_persistent_stem_pool_few_workgroups(wgs):
    """one workgroup walks all 24 tiles (five walk 5, 5, 5, 5 and 4): every tile edge, the step from one image to the next and the end of
    the walk pass through the prefetch of the next tile and both LDS images"""
    from aldi_amd import _lib as L
    L.set_tuning("stem_pool_wgs", wgs)
    got, ref = _stem_both([(64, 96), (64, 96)], 5)
    assert torch.equal(got, ref)


def _bneck_operands(N, H, W, seed, shift_bias):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, 64, generator=g).to(torch.bfloat16).to(DEV)
    w1 = torch.randn(64, 1, 1, 64, generator=g) / 8.0
    w2 = torch.randn(64, 3, 3, 64, generator=g) / 24.0
    w3 = torch.randn(256, 1, 1, 64, generator=g) / 8.0
    wsc = (torch.randn(256, 1, 1, 64, generator=g) / 8.0).to(torch.bfloat16).to(DEV).contiguous()
    s = [(torch.rand(c, generator=g) + 0.5).to(DEV) for c in (64, 64, 256)]
    b = [(torch.randn(c, generator=g) * 0.3).to(DEV) for c in (64, 64, 256)]
    ssc = (torch.rand(256, generator=g) + 0.5).to(DEV)
    bsc = (torch.randn(256, generator=g) * 0.3 + shift_bias).to(DEV)
    return x, [w.to(DEV).contiguous() for w in (w1, w2, w3)], s, b, wsc, ssc, bsc


# the tile is 8 x 16 pixels: exactly one; ragged in both directions over several images; several tiles with ragged edges.
# shift_bias -2: the shortcut's shift pulls the sum below zero, most outputs are clipped by the final ReLU
@pytest.mark.parametrize("N,H,W,shift_bias", [(1, 8, 16, 0.0), (3, 21, 19, 0.0), (2, 37, 50, 0.0), (3, 21, 19, -2.0)])
def test_bottleneck_with_shortcut_equals_two_launches(N, H, W, shift_bias):
    from aldi_amd import _lib as L, ops
    x, ws, s, b, wsc, ssc, bsc = _bneck_operands(N, H, W, H * 100 + W, shift_bias)
    plan = ops.FoldWeightsPlan(list(zip(ws, s)))
    plan.run()
    sc = ops.conv2d(x, wsc, scale=ssc, shift=bsc)
    want = ops.bottleneck_fused(x, sc, *plan.out, *b)
    got = ops.bottleneck_fused(x, x, *plan.out, *b, shortcut=(wsc, ssc, bsc))
    torch.cuda.synchronize()
    assert "shortcut" in L.last_dispatch()
    clipped = float((want == 0).float().mean())
    assert 0.02 < clipped < 0.98 and (shift_bias == 0 or clipped > 0.6), clipped        # (of the inputs: both sides of the ReLU are exercised)
    assert torch.equal(got, want)


def test_trunk_with_shortcut_fold_equals_trunk_without():
    """P2..P6 of the bf16 trunk with res2.0's shortcut inside the bottleneck kernel == the same trunk with the shortcut as its own launch"""
    from aldi_amd import synthetic as syn
    from aldi_amd.arch import ParamLayout
    from aldi_amd.engine import RCNN, Weights
    K, H, W = 8, 192, 256
    lay = ParamLayout(K)
    w = Weights(lay, torch.device(DEV), torch.bfloat16, trainable=True)
    w.load_state_dict(syn.init_state_dict(K, seed=1))
    m = RCNN(w, K)
    assert m.knobs.fused_res2 and m.knobs.fused_res2_shortcut
    _, data, _, _ = syn.make_batch(2, 0, H, W, K, seed=0)
    st, sizes, _ = m.stage_images([d["image"] for d in data])
    outs = {}
    for fold in (True, False):
        with m.with_knobs(fused_res2_shortcut=fold):
            c = m.trunk(st, sizes, save=False)
        torch.cuda.synchronize()
        outs[fold] = c.P
    assert len(outs[True]) == 5 and float(outs[False][0].float().abs().max()) > 0
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)

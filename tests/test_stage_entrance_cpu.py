"""The pair form of the 1x1 igemm (csrc/igemm_pair.h) without a GPU: the plan query on the workload's stage entrances and on combinations it
must refuse, and the generated code's scratch size."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 0x1000          # any non-null pointer: the plan never dereferences one


def _args(N, Ho, Wo, K, Cout, *, bits=False, dtype=None, **over):
    from aldi_amd import _lib as L
    f = dict(x=P, w=P, y=P, y_f32=None, scale=P, shift=P, res=None, mask=None, N=N, H=Ho, W=Wo, Cin=K, Cout=Cout, KH=1, KW=1, stride=1, pad=0,
             Ho=Ho, Wo=Wo, relu=1, res_mode=0, out_scale=1, OH=0, OW=0, dtype=L.BF16 if dtype is None else dtype, ws=None, ksplit=0, mask_bits=None,
             bits_out=P if bits else None)
    f.update(over)
    return L.ConvArgs(**f)


def _pre(H2, W2, Cin2, stride2, rounding=0, affine=True):
    from aldi_amd import _lib as L
    return L.ConvPreArgs(P, P, P if affine else None, P if affine else None, H2, W2, Cin2, stride2, rounding)


# the 1333 x 800 workload (800 x 1344 padded): C2 200 x 336 x 256, C3 100 x 168 x 512, C4 50 x 84 x 1024, C5 25 x 42 x 2048
ENTRANCES = [(200, 336, 256, 128, 512), (100, 168, 512, 256, 1024), (50, 84, 1024, 512, 2048)]      # H, W, channels of the stage input; mid; 4 * mid


@pytest.mark.parametrize("N,save", [(4, True), (2, False)])
@pytest.mark.parametrize("H2,W2,Cin2,mid,Cout", ENTRANCES)
def test_plan_names_the_pair_kernel_for_the_forward_entrances(H2, W2, Cin2, mid, Cout, N, save):
    """student (N = 4, ReLU bits saved) and teacher (N = 2): conv3 + shortcut of res3.0 / res4.0 / res5.0; the unfused conv3 takes a direct
    epilogue at these sizes, so the pair rounds once"""
    from aldi_amd import _lib as L
    L.reset_tuning()
    name = L.plan_pair_dispatch(_args(N, H2 // 2, W2 // 2, mid, Cout, bits=save), _pre(H2, W2, Cin2, 2))
    assert name == "igemm_pair<bf16,128,64,4,1,pipe,tap,round1>", name


@pytest.mark.parametrize("Ho,Wo,mid,Cout_blk,Cin_stage", [(25, 42, 512, 2048, 1024), (50, 84, 256, 1024, 512)])
def test_plan_names_the_pair_kernel_for_the_backward_pairs(Ho, Wo, mid, Cout_blk, Cin_stage):
    """d/d(C4) and d/d(C3) on the compact grid: main = g1 x wt(conv1), inner = g x wt(shortcut), no scale / shift / ReLU, two roundings"""
    from aldi_amd import _lib as L
    L.reset_tuning()
    a = _args(4, Ho, Wo, mid, Cin_stage, scale=None, shift=None, relu=0)
    name = L.plan_pair_dispatch(a, _pre(Ho, Wo, Cout_blk, 1, rounding=2, affine=False))
    assert name == "igemm_pair<bf16,128,64,4,1,pipe,tap,round2>", name


def test_rounding_follows_the_unfused_launch():
    """rounding 0: the staged epilogue (igemm_direct 0) rounds twice, the direct ones once"""
    from aldi_amd import _lib as L
    a, q = _args(2, 6, 8, 512, 2048), _pre(12, 16, 1024, 2)
    try:
        L.set_tuning("igemm_direct", 0)
        assert "round2" in L.plan_pair_dispatch(a, q)
        L.reset_tuning()
        L.set_tuning("igemm_force", 2)
        assert "round1" in L.plan_pair_dispatch(a, q)
    finally:
        L.reset_tuning()


@pytest.mark.parametrize("what", ["Cout", "fp32", "3x3", "grid", "Cin2", "mask_bits", "res", "stride"])
def test_plan_refuses_what_the_pair_kernel_does_not_take(what):
    from aldi_amd import _lib as L
    L.reset_tuning()
    a, q = _args(2, 6, 8, 512, 2048), _pre(12, 16, 1024, 2)
    assert L.plan_pair_dispatch(a, q).startswith("igemm_pair<")
    if what == "Cout":
        a.Cout = 2048 + 32
    elif what == "fp32":
        a.dtype = L.F32
    elif what == "3x3":
        a.KH = a.KW = 3
        a.pad = 1
    elif what == "grid":
        q.H2 = 14                       # (14 - 1) / 2 + 1 = 7 rows, the output has 6
    elif what == "Cin2":
        q.Cin2 = 1024 + 16
    elif what == "mask_bits":
        a.mask_bits = P
        a.scale = a.shift = None
    elif what == "res":
        a.res, a.res_mode = P, 1
    elif what == "stride":
        a.stride, a.H, a.W = 2, 12, 16
    with pytest.raises(L.AldiHipError, match="conv_pair_igemm: takes bf16"):
        L.plan_pair_dispatch(a, q)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_pair_kernels_do_not_spill():
    """both instantiations use no scratch: a spilled register would be a vector-memory operation inside a loop of counted `vmcnt` waits"""
    import isa_hazard_check as H
    sizes = H.scratch_sizes(os.path.join(ROOT, "aldi_amd", "csrc", "igemm.hip"))
    pair = {k: v for k, v in sizes.items() if "igemm_pair_kernel" in k}
    assert len(pair) == 2, sorted(sizes)
    assert not any(pair.values()), pair

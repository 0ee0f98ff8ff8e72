"""The frozen prefix held to torch.equal against CPU references: the three forms of the res2 bottleneck kernel (csrc/bneck.hip), the
fp32 and the matrix-core stem, the max-pool and the persistent stem + pool kernel (csrc/elementwise.hip).  The operands
(frozen_prefix_exact.py) are built so that the answer depends neither on the order of a sum nor on where a rounding falls; their
preconditions, and that they tell the classic errors apart, are checked on the CPU in test_frozen_prefix_exact_cpu.py.  A failure names
the pixels."""
import pytest
import torch

import frozen_prefix_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _default_knobs():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _run_bottleneck(kind, form, shape, xcd):
    from aldi_amd import _lib as L, ops
    op, want = X.bneck_case(kind, form, shape)
    L.set_tuning("igemm_xcd", xcd)          # the remap of tiles to XCDs, for tile counts below 8 and not a multiple of 8
    ws = [w.to(DEV).contiguous() for w in op["w"]]
    ss = [s.to(DEV) for s in op["s"]]
    plan = ops.FoldWeightsPlan(list(zip(ws, ss)))          # as the trunk folds them
    plan.run()
    for o, w, s in zip(plan.out, op["w"], op["s"]):
        assert torch.equal(o.cpu(), X.fold(w, s)), "folded weights: bf16(w * scale)"
    x = op["x"].to(DEV).contiguous()
    b = [t.to(DEV) for t in op["b"]]
    out = torch.full((op["N"], op["H"], op["W"], 256), float("nan"), dtype=torch.bfloat16, device=DEV)      # an unwritten pixel cannot pass
    if "wsc" in op:
        got = ops.bottleneck_fused(x, x, *plan.out, *b, out=out, shortcut=(op["wsc"].to(DEV).contiguous(), op["ssc"].to(DEV), op["bsc"].to(DEV)))
    else:
        got = ops.bottleneck_fused(x, op["res"].to(DEV).contiguous(), *plan.out, *b, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    name = L.last_dispatch()
    assert f"bottleneck_fused<bf16,{op['Cin']}," in name and ("shortcut" in name) == ("wsc" in op), name
    report = X.mismatch_report(got, want, f"bottleneck {form} {kind} N,H,W={shape} igemm_xcd={xcd}")
    if report:
        print(report)
    equal = torch.equal(got.cpu(), want)
    assert equal, report


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("shape", X.BNECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(X.BNECK_FORMS))
def test_bottleneck_integer_lattice(form, shape, xcd):
    """every term of every sum is an integer: a dropped, doubled or misplaced tap, k-step, halo pixel or residual changes the result"""
    _run_bottleneck("lattice", form, shape, xcd)


@pytest.mark.parametrize("xcd", [0, 1])
@pytest.mark.parametrize("shape", X.BNECK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(X.BNECK_FORMS))
def test_bottleneck_single_term_sums(form, shape, xcd):
    """real operands, one product per sum: every rounding of the three epilogues and of the shortcut (two fp32 roundings, then bf16), to
    nearest even, with planted ties"""
    _run_bottleneck("single", form, shape, xcd)


def _check_all(pairs):
    """every (got, want, what) is held to torch.equal; all of the mismatches are reported, not only the first"""
    reports = [r for r in (X.mismatch_report(got, want, what) for got, want, what in pairs) if r]
    if reports:
        print("\n".join(reports))
    equal = all(torch.equal(got.cpu(), want) for got, want, _ in pairs)
    assert equal, "\n".join(reports)


@pytest.mark.parametrize("size_idx", range(len(X.STEM_SIZES)), ids=lambda i: "+".join(f"{h}x{w}" for h, w in X.STEM_SIZES[i]))
@pytest.mark.parametrize("name", X.STEM_SETS)
def test_stem_pool_entry_points(name, size_idx):
    """the fp32 stem (VALU), the bf16 stem (matrix cores) and max-pool, and the persistent stem + pool kernel at its default grid and
    with one workgroup walking every tile"""
    from aldi_amd import _lib as L, ops
    img, sizes, ws, refs = X.stem_case(name, size_idx)
    imgd = img.to(DEV)
    w, scale, shift = ws["w"].to(DEV).contiguous(), ws["scale"].to(DEV), ws["shift"].to(DEV)
    what = f"{name} sizes={sizes}"
    y32 = ops.stem_forward(imgd, sizes, w, scale, shift, ws["mean"], ws["std"], torch.float32)
    p32 = ops.maxpool3s2(y32)
    y16 = ops.stem_forward(imgd, sizes, w, scale, shift, ws["mean"], ws["std"], torch.bfloat16)
    p16 = ops.maxpool3s2(y16)
    wpk = ops.stem_pack_weights(w)
    fused = ops.stem_pool_forward(imgd, sizes, wpk, scale, shift, ws["mean"], ws["std"])
    L.set_tuning("stem_pool_wgs", 1)
    fused1 = ops.stem_pool_forward(imgd, sizes, wpk, scale, shift, ws["mean"], ws["std"])
    torch.cuda.synchronize()
    _check_all([(y32, refs[torch.float32][0], "stem_forward fp32 " + what),
                (p32, refs[torch.float32][1], "maxpool3s2 fp32 " + what),
                (y16, refs[torch.bfloat16][0], "stem_forward bf16 " + what),
                (p16, refs[torch.bfloat16][1], "maxpool3s2(stem_forward bf16) " + what),
                (fused, refs[torch.bfloat16][1], "stem_pool_forward " + what),
                (fused1, refs[torch.bfloat16][1], "stem_pool_forward stem_pool_wgs=1 " + what)])

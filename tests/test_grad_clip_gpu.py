"""Gradient clipping on the device for the flat SGD state: per-segment norms (exact on lattice data, 1 ulp on random data,
bit-reproducible), the coefficients (torch's three fp32 operations), the clipped update against clip_grad_* + SGD in fp64, and the
trainer with SOLVER.CLIP_GRADIENTS on and off."""
import os
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
INF = float("inf")
K, H, W = 8, 192, 256
LR, MU, WD = 0.05, 0.9, 1e-4
EPS = 2.0 ** -24                     # one fp32 rounding, relative


def _segments(ch, gap=(5, 2, 9, 1, 3, 66, 7, 130, 11)):
    """segments of the lengths at which the kernels change path, starts at offsets = 1, 2, 3 (mod 4), gaps between them"""
    lens = [1, 3, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 5]
    segs, pos = [], 0
    for i, (n, g) in enumerate(zip(lens, gap)):
        pos += g
        while pos % 4 != (1, 2, 3)[i % 3]:
            pos += 1
        segs.append((pos, n))
        pos += n
    return segs, pos + 37


@pytest.fixture(scope="module")
def table():
    from aldi_amd import ops
    segs, n = _segments(ops.CLIP_CHUNK)
    assert n <= 65536 and sorted({s % 4 for s, _ in segs}) == [1, 2, 3]
    return segs, n, ops.ClipPlan(segs, n, DEV)


def _gap_mask(segs, n):
    m = torch.ones(n, dtype=torch.bool)
    for s, ln in segs:
        m[s: s + ln] = False
    return m


def _lattice(segs, n, seed=0):
    """NaN outside the segments.  Segment i of length L: q*q elements of +-3u and q*q of +-4u (q = floor(sqrt(L/2)), u = 2^(i%5 - 2)) at
    random places, zeros elsewhere: the sum of squares 25 q^2 u^2 is exact in any order and the L2 norm 5 q u is an fp32 number."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.full((n,), float("nan"))
    exact = []
    for i, (s, ln) in enumerate(segs):
        u = 2.0 ** (i % 5 - 2)
        q = int((ln // 2) ** 0.5)
        while (q + 1) * (q + 1) * 2 <= ln:
            q += 1
        v = torch.zeros(ln)
        if q == 0:
            v[0] = 3 * u
            exact.append(3 * u)
        else:
            v[: q * q] = 3 * u
            v[q * q: 2 * q * q] = 4 * u
            exact.append(5 * q * u)
        v = v * (torch.randint(0, 2, (ln,), generator=gen) * 2 - 1)
        g[s: s + ln] = v[torch.randperm(ln, generator=gen)]
    return g, torch.tensor(exact, dtype=torch.float32)


def _random(segs, n, seed, nan_gaps=True):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    if nan_gaps:
        g[_gap_mask(segs, n)] = float("nan")
    return g


def _cpu_norms(g, segs, norm_type):
    """fp64 on the CPU, rounded once to fp32; and the global norm"""
    g = g.double()
    if norm_type == INF:
        per = torch.stack([g[s: s + ln].abs().max() for s, ln in segs])
        return per.float(), per.max().float()
    sq = torch.stack([(g[s: s + ln] ** 2).sum() for s, ln in segs])
    return sq.sqrt().float(), sq.sum().sqrt().float()


def _within_1ulp(a, r):
    a, r = a.cpu(), r.cpu()
    up, dn = torch.nextafter(r, torch.full_like(r, INF)), torch.nextafter(r, torch.full_like(r, -INF))
    return bool(((a == r) | (a == up) | (a == dn)).all())


def _cpu_coef(norm, clip_value, gscale):
    """clip_grad_norm_'s operations on fp32 tensors: clip_coef = max_norm / (total_norm + 1e-6); clamp(max=1.0)"""
    t = norm * torch.tensor(abs(gscale), dtype=torch.float32)
    return torch.clamp(clip_value / (t + 1e-6), max=1.0)


# ---- 1. norms, exact
def test_norms_exact_on_lattice_data_and_never_read_outside_their_segment(table):
    from aldi_amd import ops
    segs, n, plan = table
    g, exact = _lattice(segs, n)
    ref, _ = _cpu_norms(g, segs, 2.0)
    assert torch.equal(ref, exact)                                  # the construction: every norm IS an fp32 number
    got = ops.grad_seg_norms(g.to(DEV), plan, 2.0).cpu()
    assert torch.equal(got, ref), (got, ref)
    # inf norm: a max is exact on any data
    for seed in (1, 2):
        gr = _random(segs, n, seed)
        ref, gref = _cpu_norms(gr, segs, INF)
        got = ops.grad_seg_norms(gr.to(DEV), plan, INF, full_model=True).cpu()
        assert torch.equal(got, ref) and torch.equal(plan.global_norm.cpu(), gref.reshape(1))
    got = ops.grad_seg_norms(g.to(DEV), plan, INF).cpu()
    assert torch.equal(got, _cpu_norms(g, segs, INF)[0])


# ---- 2. norms, random data
@pytest.mark.parametrize("seed", [3, 4])
def test_l2_norms_of_random_data_within_one_ulp(table, seed):
    """every product and every sum in double: the only error is the double summation, n * 2^-53 relative, far below half an fp32 ulp,
    so the fp32 result is float32(sqrt(fp64 sum)) or its neighbour"""
    from aldi_amd import ops
    segs, n, plan = table
    g = _random(segs, n, seed)
    ref, gref = _cpu_norms(g, segs, 2.0)
    got = ops.grad_seg_norms(g.to(DEV), plan, 2.0, full_model=True)
    assert torch.isfinite(got).all()
    assert _within_1ulp(got, ref), (got.cpu(), ref)
    assert _within_1ulp(plan.global_norm, gref.reshape(1)), (plan.global_norm.cpu(), gref)


# ---- 3. reproducibility
def test_norms_are_bit_reproducible(table):
    """(the launch geometry is the chunk table's: no tuning knob changes it)"""
    from aldi_amd import ops
    segs, n, plan = table
    g = _random(segs, n, 5).to(DEV)
    other = ops.ClipPlan(segs, n, DEV)                              # workspaces of its own
    for nt in (2.0, INF):
        a = ops.grad_seg_norms(g, plan, nt, full_model=True).clone()
        ga = plan.global_norm.clone()
        plan.partials.fill_(float("nan"))                           # whatever the workspace held before
        b = ops.grad_seg_norms(g, plan, nt, full_model=True).clone()
        c = ops.grad_seg_norms(g, other, nt, full_model=True)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ga, plan.global_norm) and torch.equal(ga, other.global_norm)


# ---- 4. coefficients
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_coefficients_are_torchs_three_fp32_operations(table, gscale):
    from aldi_amd import ops
    segs, n, plan = table
    clip_value = 30.0
    g, exact = _lattice(segs, n)
    ref = _cpu_coef(exact, clip_value, gscale)
    assert bool((ref < 1).any()) and bool((ref == 1).any())
    ops.grad_seg_norms(g.to(DEV), plan, 2.0)
    assert torch.equal(ops.clip_coef(plan, clip_value, gscale).cpu(), ref)
    assert torch.equal(ops.clip_coef(plan, clip_value, -gscale).cpu(), ref)            # |gscale|
    # one inf: norm inf, coefficient exactly 0;  one NaN: both NaN
    g2 = g.clone()
    g2[segs[2][0] + 7] = INF
    g2[segs[5][0] + 1000] = float("nan")
    norm2 = exact.clone()
    norm2[2], norm2[5] = INF, float("nan")
    ref2 = _cpu_coef(norm2, clip_value, gscale)
    assert float(ref2[2]) == 0.0 and bool(torch.isnan(ref2[5])) and int(torch.isnan(ref2).sum()) == 1
    got_norm = ops.grad_seg_norms(g2.to(DEV), plan, 2.0).cpu()
    torch.testing.assert_close(got_norm, norm2, rtol=0, atol=0, equal_nan=True)
    got = ops.clip_coef(plan, clip_value, gscale).cpu()
    torch.testing.assert_close(got, ref2, rtol=0, atol=0, equal_nan=True)
    assert float(got[2]) == 0.0
    # the inf norm keeps a NaN too
    got_norm = ops.grad_seg_norms(g2.to(DEV), plan, INF).cpu()
    assert float(got_norm[2]) == INF and bool(torch.isnan(got_norm[5])) and int(torch.isnan(got_norm).sum()) == 1
    # full_model: one coefficient, from the global norm
    ops.grad_seg_norms(g.to(DEV), plan, 2.0, full_model=True)
    ref = _cpu_coef(plan.global_norm.cpu(), clip_value, gscale)
    assert float(ref) < 1
    assert torch.equal(ops.clip_coef(plan, clip_value, gscale, full_model=True).cpu(), ref.expand(len(segs)))


# ---- 5. / 6. the update
def _ref_step(p, buf, g, segs, spec, gscale, first, lr=LR, mu=MU, wd=WD):
    """clip_grad_value_ / clip_grad_norm_ on the per-segment views (all of them at once for full_model), then the SGD formula of
    sgd_kernel, all in fp64.  -> new p, new buf, their bounds, the per-segment coefficient the clip applied (norm types).

    The bound: 8 * 2^-24 * (|p| + lr * (|mu*buf| + |g*coef| + |wd*p|)), without the |p| term for the momentum buffer.  Every fp32
    operation rounds by at most 2^-24 relative.  With the gradient scale a power of two (norm * |gscale| and g * gscale exact), the
    term that passes through most of them, g*coef, sees three operations in the coefficient (+ 1e-6, the reciprocal, * clip_value)
    and five in the update (* coef, + wd*p, + mu*buf, * lr, p - ...): eight, each relative to a partial sum no larger than the sum
    of the magnitudes above.  The other terms see fewer.  (The norm's own rounding to fp32 is a ninth on that one term; all nine
    would have to fall the same way at their maximum to reach the bound.  The tests print the worst error / bound they see.)"""
    p64, b64, g64 = p.double(), buf.double(), g.double() * gscale
    params = []
    for s, ln in segs:
        q = torch.nn.Parameter(torch.zeros(ln, dtype=torch.float64))
        q.grad = g64[s: s + ln].clone()
        params.append(q)
    if spec is None:
        pass
    elif spec.clip_type == "value":
        for q in params:
            torch.nn.utils.clip_grad_value_(q, spec.clip_value)
    elif spec.clip_type == "norm":
        for q in params:
            torch.nn.utils.clip_grad_norm_(q, spec.clip_value, norm_type=spec.norm_type)
    else:
        torch.nn.utils.clip_grad_norm_(params, spec.clip_value, norm_type=spec.norm_type)
    gc = g64.clone()
    coef = []
    for q, (s, ln) in zip(params, segs):
        gc[s: s + ln] = q.grad
        den = g64[s: s + ln].abs().max()
        coef.append(float(q.grad.abs().max() / den) if float(den) > 0 else 1.0)
    d = gc + wd * p64
    mb = torch.zeros_like(b64) if first else mu * b64
    b = mb + d
    mag = mb.abs() + gc.abs() + (wd * p64).abs()
    return p64 - lr * b, b, 8 * EPS * (p64.abs() + lr * mag), 8 * EPS * mag, coef


def _specs():
    from aldi_amd.ops import ClipSpec
    return {"value": ClipSpec("value", 0.4, 2.0), "norm2": ClipSpec("norm", 6.0, 2.0), "norminf": ClipSpec("norm", 1.2, INF),
            "full_model": ClipSpec("full_model", 10.0, 2.0), "full_model_inf": ClipSpec("full_model", 1.5, INF)}


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("mode", ["value", "norm2", "norminf", "full_model", "full_model_inf"])
def test_clipped_update_vs_fp64_clip_grad_and_sgd(table, mode, bf16):
    from aldi_amd import ops
    segs, n, plan = table
    spec = _specs()[mode]
    gscale = 0.5
    dtype = torch.bfloat16 if bf16 else torch.float32
    gen = torch.Generator().manual_seed(17)
    pad = _gap_mask(segs, n)
    p = (0.3 * torch.randn(n, generator=gen)).to(DEV)
    buf = torch.zeros(n, device=DEV)
    pc = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if bf16 else None
    bit, free = 0, 0
    for it in range(3):
        first = it == 0
        g = torch.randn(n, generator=gen)
        gd = g.to(DEV)
        p_new, b_new, bound_p, bound_b, coef = _ref_step(p.cpu(), buf.cpu(), g, segs, spec, gscale, first)
        bit += sum(c < 1 for c in coef)
        free += sum(c == 1 for c in coef)
        # the unclipped kernel on a copy: what the padding must look like
        p0, buf0 = p.clone(), buf.clone()
        pc0 = pc.clone() if bf16 else None
        ops.sgd_step(p0, gd, buf0, pc0, n, LR, MU, WD, gscale, first, dtype)
        ops.sgd_step_clip(p, gd, buf, pc, plan, spec, LR, MU, WD, gscale, first, dtype)
        ep, eb = (p.cpu().double() - p_new).abs(), (buf.cpu().double() - b_new).abs()
        print("%s bf16=%d step %d: max err/bound p %.3f buf %.3f" % (mode, bf16, it, float((ep / bound_p).max()), float((eb / bound_b).max())))
        assert bool((ep <= bound_p).all()), float((ep / bound_p).max())
        assert bool((eb <= bound_b).all()), float((eb / bound_b).max())
        assert torch.equal(p[pad.to(DEV)], p0[pad.to(DEV)]) and torch.equal(buf[pad.to(DEV)], buf0[pad.to(DEV)])
        if bf16:
            assert torch.equal(pc, p.to(torch.bfloat16))
            assert torch.equal(pc[pad.to(DEV)], pc0[pad.to(DEV)])
        if mode != "value":                                          # the clip must have changed something the unclipped step did not
            assert not torch.equal(p, p0)
    if spec.clip_type == "norm":
        assert bit > 0 and free > 0, (bit, free)                     # the reference itself clips some parameters and leaves others
    else:
        assert bit > 0


@pytest.mark.parametrize("mode", ["value", "norm"])
def test_a_clip_that_never_bites_is_the_unclipped_step(table, mode):
    """value above every |g|, norm at 1e30: within the same bound of aldi_sgd_step (no bit identity claimed)"""
    from aldi_amd import ops
    from aldi_amd.ops import ClipSpec
    segs, n, plan = table
    gen = torch.Generator().manual_seed(23)
    g = torch.randn(n, generator=gen)
    spec = ClipSpec("value", float(g.abs().max()) * 2, 2.0) if mode == "value" else ClipSpec("norm", 1e30, 2.0)
    for bf16 in (False, True):
        dtype = torch.bfloat16 if bf16 else torch.float32
        p = (0.3 * torch.randn(n, generator=gen)).to(DEV)
        buf = torch.randn(n, generator=gen).to(DEV)
        pc = torch.zeros(n, dtype=torch.bfloat16, device=DEV) if bf16 else None
        _, _, bound_p, bound_b, _ = _ref_step(p.cpu(), buf.cpu(), g, segs, None, 1.0, False)
        p0, buf0, pc0 = p.clone(), buf.clone(), (pc.clone() if bf16 else None)
        ops.sgd_step(p0, g.to(DEV), buf0, pc0, n, LR, MU, WD, 1.0, False, dtype)
        ops.sgd_step_clip(p, g.to(DEV), buf, pc, plan, spec, LR, MU, WD, 1.0, False, dtype)
        assert not torch.equal(p0.cpu(), p.cpu() * 0)
        assert bool(((p.cpu().double() - p0.cpu().double()).abs() <= bound_p).all())
        assert bool(((buf.cpu().double() - buf0.cpu().double()).abs() <= bound_b).all())
        if bf16:
            assert torch.equal(pc, p.to(torch.bfloat16))


# ---- 7. / 8. the trainer
def _cfg(align, bf16=False, lr=0.002):
    """the smallest configuration of tests/test_engine_gpu.py"""
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.AMP.ENABLED", bf16, "SOLVER.BASE_LR", lr, "SOLVER.WARMUP_ITERS", 0, "SEED", 1,
                         "EMA.ALPHA", 0.9, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W,
                         "DOMAIN_ADAPT.ALIGN.IMG_DA_ENABLED", bool(align), "DOMAIN_ADAPT.ALIGN.INS_DA_ENABLED", bool(align),
                         "SOLVER.FUSED_STEP", False, "SOLVER.STEP_GRAPH", False])
    return cfg


def _run(cfg, iters, inject=None):
    """an identically seeded trainer; optimizer.step wrapped to snapshot the state it is about to update (inject: a gradient per iteration
    that replaces the one the backward left, just before the step).
    -> trainer, [(grad, master, mom, gscale, first_step, _sgd_applied, master after the step)], [_defers_sgd() per iteration]"""
    from aldi_amd.trainer import ALDITrainer
    random.seed(0)
    torch.manual_seed(11)
    tr = ALDITrainer(cfg)
    Wt, opt, n = tr.model.weights, tr._trainer.optimizer, tr.model.layout.n_train
    rec = []
    orig = opt.step

    def step():
        if inject is not None:
            Wt.grad.copy_(inject[len(rec)])
        snap = [Wt.grad.cpu().clone(), Wt.master[:n].cpu().clone(), Wt.mom.cpu().clone(), float(getattr(Wt, "_gscale", 1.0)), bool(Wt.first_step),
                bool(getattr(Wt, "_sgd_applied", False))]
        orig()
        rec.append(snap + [Wt.master[:n].cpu().clone()])
    opt.step = step
    defers = []
    for it in range(iters):
        tr.iter = it
        tr.before_step()
        defers.append(tr._trainer._defers_sgd())
        tr.run_step()
        tr.after_step()
    torch.cuda.synchronize()
    return tr, rec, defers


@pytest.fixture(scope="module")
def unclipped_run():
    """two iterations with the node present and ENABLED False: the dry run of case 7 and one side of case 8"""
    cfg = _cfg(False)
    cfg.SOLVER.FUSED_STEP = True
    assert cfg.SOLVER.CLIP_GRADIENTS.ENABLED is False
    tr, rec, _ = _run(cfg, 2)
    assert tr._trainer.optimizer.clip is None
    return tr.model.layout, [r[0] for r in rec], [r[-1] for r in rec]


@pytest.mark.parametrize("in_step", ["0", "1"])
def test_trainer_clips_per_parameter_like_detectron2(unclipped_run, in_step, monkeypatch):
    from aldi_amd.ops import ClipSpec
    lay, dry_grads, _ = unclipped_run
    segs = [(off, numel) for _, off, numel in lay.param_segments()]
    norms0, _ = _cpu_norms(dry_grads[0], segs, 2.0)
    clip_value = float(norms0.median())
    assert clip_value > 0
    monkeypatch.setenv("ALDI_SGD_IN_STEP", in_step)
    cfg = _cfg(False)
    cfg.SOLVER.FUSED_STEP = True
    cfg.SOLVER.CLIP_GRADIENTS.ENABLED = True
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_TYPE = "norm"
    cfg.SOLVER.CLIP_GRADIENTS.CLIP_VALUE = clip_value
    tr, rec, defers = _run(cfg, 2)
    spec = tr._trainer.optimizer.clip
    assert spec == ClipSpec("norm", clip_value, 2.0)
    assert getattr(tr._trainer, "_fused_step", None) is not None                      # the fused step ran
    assert defers == [False, False]                                  # ALDI_SGD_IN_STEP=1 cannot bypass the clip
    lr = tr._trainer.optimizer.param_groups[0]
    for it, (g, p, mom, gscale, first, applied, p_after) in enumerate(rec):
        assert first == (it == 0) and not applied and gscale == 1.0
        p_new, _, bound_p, _, coef = _ref_step(p, mom, g, segs, spec, gscale, first, lr=lr["lr"], mu=lr["momentum"], wd=lr["weight_decay"])
        bit = sum(c < 1 for c in coef)
        print("iteration %d: clipped %d of %d parameters" % (it, bit, len(coef)))
        if it == 0:
            assert 0.25 * len(coef) <= bit <= 0.75 * len(coef), (bit, len(coef))    # the median of the dry run: about half
        err = (p_after.double() - p_new).abs()
        assert bool((err <= bound_p).all()), float((err / bound_p).max())
        assert not torch.equal(p_after, p)
    ref, _ = _cpu_norms(rec[-1][0], segs, 2.0)
    got = tr.model.weights.grad_norms()
    assert got.is_cuda and got.shape == (len(segs),)
    assert _within_1ulp(got, ref)


def test_clipping_disabled_is_the_trainer_without_the_node(unclipped_run, monkeypatch):
    """Two iterations with ENABLED False against two with no CLIP_GRADIENTS node: the same optimizer object, the same launches, the same
    bits.  The engine's backward is not reproducible from run to run (float atomics where layers share a gradient buffer): two trainers
    built from the SAME node-less config differ in 4.5 M gradient elements after iteration 0 (max 4.8e-07 at max|g| 3.4) and in 28 k
    master elements (3.0e-08), 3.2 M (2.7e-07) after iteration 1 -- exactly as much as ENABLED False differs from no node (4.6 M / 28 k,
    2.1 M).  So both trainers step on the same gradients: the node-less one takes, just before each optimizer step, the gradient the
    other one stepped on.  Everything else of its iterations runs as it is, and the masters must then be equal bit for bit."""
    from aldi_amd import ops
    _, grads, with_node = unclipped_run
    cfg = _cfg(False)
    cfg.SOLVER.FUSED_STEP = True
    del cfg.SOLVER["CLIP_GRADIENTS"]
    assert "CLIP_GRADIENTS" not in cfg.SOLVER

    def never(*a, **kw):
        raise AssertionError("the clipped step must not run")
    calls = []
    plain = ops.sgd_step
    monkeypatch.setattr(ops, "sgd_step_clip", never)
    monkeypatch.setattr(ops, "grad_seg_norms", never)
    monkeypatch.setattr(ops, "sgd_step", lambda *a, **kw: (calls.append(1), plain(*a, **kw))[1])
    tr, rec, _ = _run(cfg, 2, inject=grads)
    assert type(tr._trainer.optimizer).__name__ == "EngineSGD" and tr._trainer.optimizer.clip is None
    assert len(calls) == 2 and getattr(tr.model.weights, "_clip_plan", None) is None
    for a, b in zip(with_node, rec):
        assert torch.equal(a, b[-1])

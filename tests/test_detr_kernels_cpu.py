"""The references of tests/detr_kernel_refs.py pinned without a GPU: the lattice operands meet their exactness preconditions, the
explicit fp64 statement of multi-scale deformable attention equals oracle/ms_deform_attn.py (fp32 and fp64 alike) except for the location
gradient of samples exactly at -1, and every fp64-matched reference equals torch autograd or the oracle."""
import pytest
import torch
import torch.nn.functional as F

import detr_kernel_refs as R


def _oracle(ops, shapes, dtype):
    from oracle.ms_deform_attn import ms_deform_attn
    v, l, w = (ops[k].detach().clone().to(dtype).requires_grad_(True) for k in ("value", "loc", "attw"))
    out = ms_deform_attn(v, list(shapes), l, w)
    out.backward(ops["gout"].to(dtype))
    return out.detach(), v.grad, l.grad, w.grad


@pytest.mark.parametrize("i", range(len(R.MSDA_CASES)))
def test_lattice_operands_are_exact_and_the_reference_is_the_oracle(i):
    N, M, D, Lq, shapes, P = R.MSDA_CASES[i]
    ops, ref, st = R.msda_case(i)                       # (check_lattice ran: magnitudes, sample mix, edges where a sixteenth reaches them)
    o64, o32 = _oracle(ops, shapes, torch.float64), _oracle(ops, shapes, torch.float32)
    for a, b in zip(o64, o32):                          # the order of a sum and the width of the format do not matter on these operands
        assert torch.equal(a, b.double())
    assert torch.equal(ref[0], o64[0]) and torch.equal(ref[1], o64[1]) and torch.equal(ref[3], o64[3])
    # the location gradient: grid_sample's rule differentiates through the corner at 0 of a sample exactly at -1, the extension's rule
    # (the kernel's) leaves the sample out -- the two differ there and nowhere else
    differ = ref[2] != o64[2]
    at_m1 = st["mask_minus_one"].any(-1, keepdim=True).expand_as(differ)
    assert not (differ & ~at_m1).any()
    assert (ref[2][at_m1] == 0).all()
    if R.has_edges(shapes):
        assert differ.any()


def test_lattice_cases_together_hold_every_edge():
    """the shares asked of every case that can have them hold for the set as a whole too (two cases have no side that divides 8)"""
    n = tot = m1 = side = 0
    for i in range(len(R.MSDA_CASES)):
        st = R.msda_case(i)[2]
        k = st["mask_minus_one"][..., 0].numel()
        tot += k
        m1 += st["minus_one"] * k
        side += st["at_side"] * k
        n += R.has_edges(R.MSDA_CASES[i][4])
    assert n >= 5 and m1 / tot >= 0.003 and side / tot >= 0.003
    assert R.edge_locs(4) == (-0.125, 1.125) and R.edge_locs(1) == (-0.5, 1.5) and R.edge_locs(6) is None


def test_first_case_counts():
    """the exception is a minority of the samples at -1: the corner at 0 must also carry a non-zero gradient"""
    ops, ref, st = R.msda_case(0)
    o64 = _oracle(ops, R.MSDA_CASES[0][4], torch.float64)
    n_m1, n_diff = int(st["mask_minus_one"].sum()), int((ref[2] != o64[2]).sum())
    assert 0 < n_diff < 2 * n_m1 and n_m1 >= 100, (n_diff, n_m1)


@pytest.mark.parametrize("name", list(R.SELF_CASES))
def test_self_attention_operands(name):
    pyr, N, M, D, P, weights, one_point = R.SELF_CASES[name]
    shapes, ops, ref, st = R.self_case(name)
    S = sum(h * w for h, w in shapes)
    assert ops["loc"].shape == (N, S, M, len(shapes), P, 2) and len(shapes) <= 8
    from oracle.ms_deform_attn import ms_deform_attn
    assert torch.equal(ms_deform_attn(ops["value"].double(), list(shapes), ops["loc"].double(), ops["attw"].double()), ref[0])
    assert ref[1].abs().max().item() >= 1.0
    share = R.near_share(ops, shapes)
    if name in ("nested", "ragged"):
        assert 0.2 < share < 0.95, share                # the walk and the far scatter both receive samples
    if one_point is not None:
        # > kSCap = 2048 samples of one head touch one pixel of the coarsest level (1 x 1 tiles there: S P / (H W) * 9 > 1500): the
        # walk's LDS list overflows; with weights <= 1/2 the pile stays below 2^14 (check_lattice asserted it)
        assert S * P > 2048 and ops["attw"].max().item() <= 0.5
        H, W = shapes[-1]
        assert R.gather_tile_logs(shapes, P, 1500)[-1] == 0
        assert R.pile_count(ops, shapes, len(shapes) - 1, W // 2, H // 2) > 2048 + 512


def test_gather_list_settings_reach_every_tile_size():
    for name in ("nested", "ragged"):
        shapes, P = R.SELF_PYRAMIDS[R.SELF_CASES[name][0]], R.SELF_CASES[name][4]
        seen = set()
        for lim in R.GATHER_LISTS:
            seen |= set(R.gather_tile_logs(shapes, P, lim))
        assert seen == {0, 1, 2, 3}, (name, seen)


# ------------------------------------------------------------------------------------------------ fp64-matched references
def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


@pytest.mark.parametrize("case", [(2, 9, 2, 16), (1, 1, 1, 16), (1, 65, 3, 32)])
@pytest.mark.parametrize("drop", [False, True])
def test_small_attention_reference_is_softmax_attention(case, drop):
    B, Q, H, Dh = case
    q, k, v, do = (t.double() for t in R.mha_operands(B, Q, H, Dh, 5))
    keep = None
    if drop:
        g = torch.Generator().manual_seed(1)
        keep = (torch.rand(B, H, Q, Q, generator=g) >= 0.1).double() / 0.9
    scale = Dh ** -0.5
    ref = R.mha_ref(q, k, v, do, H, scale, keep)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.view(B, Q, H, Dh).transpose(1, 2) for t in (qa, ka, va))
    s = (qh * scale) @ kh.transpose(-1, -2)
    p = torch.softmax(s, -1)
    out = ((p * keep if drop else p) @ vh).transpose(1, 2).reshape(B, Q, H * Dh)
    out.backward(do)
    _close(ref["out"], out.detach())
    _close(ref["lse"], torch.logsumexp(s, -1).detach())
    _close(ref["dq"], qa.grad); _close(ref["dk"], ka.grad); _close(ref["dv"], va.grad)
    _close(ref["delta"], (do * out.detach()).view(B, Q, H, Dh).sum(-1).transpose(1, 2))
    if Q == 1 and not drop:
        assert ref["dq"].abs().max() == 0 and ref["dk"].abs().max() == 0 and torch.equal(ref["dv"], do)
    if not drop:
        from oracle import deformable_detr as D
        d = H * Dh
        eye = torch.eye(d, dtype=torch.float64)
        p_ = {"a.in_proj_weight": torch.cat([eye, eye, eye]), "a.in_proj_bias": torch.zeros(3 * d, dtype=torch.float64), "a.out_proj.weight": eye,
              "a.out_proj.bias": torch.zeros(d, dtype=torch.float64)}
        _close(ref["out"], D.multihead_self_attention(p_, "a", q, k, v, H))


@pytest.mark.parametrize("case", [(2, 37, 24, 4), (1, 1, 32, 32), (3, 257, 64, 4)])
def test_group_norm_reference_is_torchs(case):
    N, HW, C, G = case
    ops = [t.double() for t in R.gn_operands(N, HW, C, G, 3)]
    ref, tor = R.gn_ref(*ops, G), R.gn_torch(*ops, G)
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        _close(ref[k], tor[k], 1e-10)
    if HW * C // G > 1:                                 # (F.group_norm refuses one value per group; native_group_norm above takes it)
        _close(ref["y"], F.group_norm(ops[0].permute(0, 2, 1), G, ops[1], ops[2], R.GN_EPS).permute(0, 2, 1), 1e-10)
    else:
        assert torch.equal(ref["y"], ops[2].expand(N, HW, C)) and torch.equal(ref["rstd"], torch.full((N, G), R.GN_EPS, dtype=torch.float64).rsqrt())


def test_group_norm_yardsticks_on_offset_inputs():
    """the two-pass reference and torch's group_norm in fp32 stay within a few 1e-6 of the fp64 truth at mean / std = 30, where one pass
    of sum(x) and sum(x^2) in fp32 loses two more digits"""
    N, HW, C, G = 1, 1961, 64, 8
    ops = R.gn_operands(N, HW, C, G, 4, offset=30.0, std=1.0)
    r32, r64 = R.both(R.gn_ref, *ops, G=G)
    t32 = R.gn_torch(*ops, G)
    for k in ("y", "dx"):
        assert (r32[k].double() - r64[k]).abs().max().item() < 2e-5 and (t32[k].double() - r64[k]).abs().max().item() < 2e-5
    x = ops[0].view(N, HW, G, C // G)
    m = x.mean((1, 3))
    naive = ((x * x).mean((1, 3)) - m * m + R.GN_EPS).rsqrt()
    assert (naive.double() - r64["rstd"].view(N, G)).abs().max().item() > 20 * (r32["rstd"].double() - r64["rstd"]).abs().max().item()


@pytest.mark.parametrize("case", R.PREPARE_CASES)
def test_sampling_glue_reference_is_the_oracles(case):
    T, M, L, P = case
    raw, ref, g_loc, g_aw = (t.double() for t in R.prepare_operands(T, M, L, P, 6))
    shapes = R.PREPARE_SHAPES
    out = R.prepare_ref(raw, ref, g_loc, g_aw, shapes, M, L, P)
    ra, fa = raw.clone().requires_grad_(True), ref.clone().requires_grad_(True)
    LP = L * P
    # oracle/deformable_detr.py, deformable_attention: lines "off = ...", "aw = ...", "loc = ..."
    off = ra[:, : M * LP * 2].view(1, T, M, L, P, 2)
    aw = F.softmax(ra[:, M * LP * 2:].view(1, T, M, LP), -1).view(1, T, M, L, P)
    normalizer = torch.tensor([[w, h] for (h, w) in shapes[:L]], dtype=torch.float64)
    loc = fa.view(1, T, L, 2)[:, :, None, :, None, :] + off / normalizer[None, None, None, :, None, :]
    ((loc[0] * g_loc).sum() + (aw[0] * g_aw).sum()).backward()
    _close(out["loc"], loc[0].detach()); _close(out["aw"], aw[0].detach())
    _close(out["g_raw"], ra.grad); _close(out["g_ref"], fa.grad)
    if LP == 1:
        assert torch.equal(out["aw"], torch.ones_like(out["aw"])) and out["g_raw"][:, M * LP * 2:].abs().max() == 0


@pytest.mark.parametrize("R_,refs", [(300, 100), (1, 1), (257, 257)])
def test_box_finish_reference_is_inverse_sigmoid_and_autograd(R_, refs):
    from oracle import deformable_detr as D
    t, ref, gb, g0 = (x.double() for x in R.box_operands(R_, refs, 8))
    out = R.box_ref(t, ref, gb, g0)
    ta, ra = t.clone().requires_grad_(True), ref.clone().requires_grad_(True)
    lo = D.inverse_sigmoid(ra)[torch.arange(R_) % refs]
    boxes = torch.sigmoid(torch.cat([ta[:, :2] + lo, ta[:, 2:]], 1))
    boxes.backward(gb)
    _close(out["boxes"], boxes.detach()); _close(out["g_t"], ta.grad)
    _close(out["g_ref"], g0 + ra.grad, 1e-9)
    if refs >= 12:
        vals = ref[:, 0]
        assert (vals == 0).any() and (vals == 1).any() and (vals < 0).any() and (vals > 1).any()
        assert ((vals > 0) & (vals < 1e-5)).any() and ((vals > 1 - 1e-5) & (vals < 1)).any()


def test_criterion_reference_is_the_oracles_criterion():
    from oracle import deformable_detr as D
    logits, boxes, targets = R.criterion_operands(11)
    lg, bx = logits.double(), boxes.double()
    tg = [{"labels": t["labels"], "boxes": t["boxes"].double()} for t in targets]
    indices = [D.hungarian_match(lg[l], bx[l], tg) for l in range(lg.shape[0])]
    ref = R.criterion_ref(lg, bx, targets, indices)
    la, ba = lg.clone().requires_grad_(True), bx.clone().requires_grad_(True)
    d, total = D.criterion(la, ba, tg)
    total.backward()
    w = torch.tensor([2.0, 5.0, 2.0], dtype=torch.float64)
    want = torch.stack([torch.stack([d[k + ("" if l == lg.shape[0] - 1 else f"_{l}")] for k in ("loss_ce", "loss_bbox", "loss_giou")]) for l in range(lg.shape[0])]).detach() * w
    _close(ref["losses"], want); _close(ref["g_logits"], la.grad); _close(ref["g_boxes"], ba.grad)
    assert torch.isfinite(ref["losses"]).all() and torch.isfinite(ref["g_logits"]).all() and torch.isfinite(ref["g_boxes"]).all()
    r32 = R.criterion_ref(logits, boxes, targets, indices)
    assert all(torch.isfinite(v).all() for v in r32.values())
    assert set(logits.unique().tolist()) == {0.0, 30.0, -30.0, 100.0, -100.0}


def test_tolerance_rule():
    a64 = torch.tensor([1.0, -2.0], dtype=torch.float64)
    a32 = torch.tensor([1.0 + 2.0 ** -20, -2.0])
    assert R.tolerance(a32, a64) == pytest.approx(8 * 2.0 ** -20 + 4 * 2.0 ** -24 * 2.0)
    assert R.tolerance(a64.float(), a64) == 4 * 2.0 ** -24 * 2.0

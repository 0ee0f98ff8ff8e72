"""Operands and plain CPU references for the kernel-level tests of the Deformable-DETR side (csrc/msda.hip, csrc/detr.hip).

Two kinds of check, as in frozen_prefix_exact.py:

  lattice operands   multi-scale deformable attention on operands for which every product and every sum is exact in fp32 in any order:
                     locations k / 16 on levels of side <= 64 (loc * W - 0.5 has <= 4 fraction bits with or without a fused multiply-add,
                     so do the bilinear fractions), weights from {0, 1/4, 1/2, 1}, integer values in [-4, 4], upstream gradients from
                     {-1, 0, 1}.  Every kernel form is then held to torch.equal with an explicit fp64 reference; samples exactly on a cell
                     boundary, at -1 and at W are part of the operands, so the kernel's conventions (x > -1 strict, x < W strict, the
                     floor cell) are pinned.  `check_lattice` asserts on the reference side that the construction really is exact.
  fp64-matched       the remaining kernels (small attention, GroupNorm, the sampling glue, the box head's last step) against ONE dtype
                     generic torch function each: the truth is that function in fp64 on the fp32 operands, the yardstick is the same function
                     in fp32 on the CPU, and a kernel may be `factor` times as far from the truth as the yardstick (`tolerance`).

Nothing here touches the library under test.  Shared by test_detr_kernels_cpu.py and test_detr_kernels_gpu.py."""
import functools

import torch

EPS_BOX = 1e-5

# ------------------------------------------------------------------------------------------------ lattice MSDA: operands
# (N, M, D, Lq, levels, P).  msda_kernel<D, true> keeps a pair's L * P results spread over its D / 4 lanes when L * P <= 2 * (D / 4)
# and stores them word by word from lane 0 otherwise.
MSDA_CASES = [
    (2, 2, 32, 300, ((7, 11), (4, 6), (13, 21), (5, 5), (3, 9)), 4),      # L * P = 20 > 16: word-by-word stores; 1200 pairs: dead pairs in the last wave
    (1, 3, 32, 77, ((5, 7), (3, 3), (9, 2)), 6),                          # L * P = 18
    (1, 2, 64, 97, ((5, 7), (3, 3), (9, 2), (1, 1), (6, 6)), 8),          # L * P = 40 > 32: word-by-word stores at D = 64
    (1, 2, 64, 33, ((6, 5), (3, 3)), 16),                                 # L * P = 32 = 2 * LANES: both spread slots full
    (2, 8, 32, 64, ((25, 42), (13, 21), (7, 11), (4, 6)), 4),             # the configuration's own 16 samples
    (1, 2, 32, 40, ((5, 7), (3, 3), (2, 9)), 3),                          # L * P = 9: the second spread slot partly used
    (1, 1, 32, 5, ((1, 1),), 1),                                          # one sample, fewer than LANES; a one-pixel level
]
WEIGHTS = (0.0, 0.25, 0.5, 1.0)


def level_starts(shapes):
    out, s = [], 0
    for h, w in shapes:
        out.append(s)
        s += h * w
    return out


def edge_locs(side):
    """the two locations, in sixteenths, whose pixel coordinate loc * side - 0.5 is exactly -1 / exactly `side`: -1 / (2 side) and
    1 + 1 / (2 side).  They exist only when the side divides 8."""
    return (-0.5 / side, 1.0 + 0.5 / side) if 8 % side == 0 else None


def has_edges(shapes):
    return any(edge_locs(s) is not None for hw in shapes for s in hw)


def _plant_edges(loc, shapes, g, rate=0.04):
    """a share of the coordinates exactly at -1 and exactly at W (H), on the levels where a sixteenth reaches them; the first three
    samples are set by hand so that a case of a handful of samples has one of each and one exactly on a pixel centre"""
    for l, (H, W) in enumerate(shapes):
        for c, side in ((0, W), (1, H)):
            e = edge_locs(side)
            if e is None:
                continue
            r = torch.rand(loc[:, :, :, l, :, c].shape, generator=g)
            sel = loc[:, :, :, l, :, c]
            sel[r < rate] = e[0]
            sel[(r >= rate) & (r < 2 * rate)] = e[1]
    flat = loc.view(-1, loc.shape[3], loc.shape[4], 2)
    for l, (H, W) in enumerate(shapes):
        for c, side in ((0, W), (1, H)):
            e = edge_locs(side)
            if e is not None and flat.shape[0] >= 3:
                flat[0, l, 0, :] = 0.5
                flat[0, l, 0, c] = e[0]
                flat[1, l, 0, :] = 0.5
                flat[1, l, 0, c] = e[1]
                flat[2, l, 0, :] = 0.5            # x = W / 2 - 1 / 2: an integer on odd sides, inside on all
                return


def lattice_msda(N, M, D, Lq, shapes, P, seed, weights=WEIGHTS):
    """-> dict(value (N, S, M, D), loc (N, Lq, M, L, P, 2), attw (N, Lq, M, L, P), gout (N, Lq, M * D)), fp32"""
    assert max(max(hw) for hw in shapes) <= 64
    g = torch.Generator().manual_seed(seed)
    S, L = sum(h * w for h, w in shapes), len(shapes)
    loc = torch.randint(-2, 19, (N, Lq, M, L, P, 2), generator=g).float() / 16
    _plant_edges(loc, shapes, g)
    attw = torch.tensor(weights)[torch.randint(0, len(weights), (N, Lq, M, L, P), generator=g)]
    value = torch.randint(-4, 5, (N, S, M, D), generator=g).float()
    gout = torch.randint(-1, 2, (N, Lq, M * D), generator=g).float()
    return dict(value=value, loc=loc, attw=attw, gout=gout)


# self attention: the queries are the pyramid's positions
SELF_PYRAMIDS = {
    "nested": ((37, 53), (19, 27), (10, 14), (5, 7)),
    "ragged": ((12, 20), (5, 9), (7, 3), (1, 1)),
    "one": ((16, 16),),
    "eight": ((9, 8), (8, 7), (7, 6), (6, 5), (5, 4), (4, 3), (3, 2), (1, 1)),     # the limit of GatherTiles / BinTiles
}
# name -> (pyramid, N, M, D, P, weights, one_point)
SELF_CASES = {
    "nested": ("nested", 2, 3, 32, 4, WEIGHTS, None),
    "ragged": ("ragged", 1, 3, 32, 4, WEIGHTS, None),
    "one": ("one", 1, 1, 32, 4, WEIGHTS, None),
    "eight": ("eight", 2, 1, 32, 2, WEIGHTS, None),
    "pile": ("nested", 1, 1, 32, 4, WEIGHTS[:3], (0.5, 0.5)),      # every query samples around one point: a tile's LDS list overflows
    "d64": ("ragged", 1, 2, 64, 2, WEIGHTS, None),                 # head dim 64: the self form hands over to the general scatter
}
GATHER_LISTS = (100000, 1500, 300, 50, 1)                          # msda_gather_list settings: between them every tile edge 8, 4, 2, 1 occurs
NEAR_PX = 5                                                       # kGR of msda.hip: the gather walk takes samples within 5 pixels of the query's centre


def self_reference_points(shapes):
    return torch.cat([torch.stack(torch.meshgrid((torch.arange(h) + 0.5) / h, (torch.arange(w) + 0.5) / w, indexing="ij"), -1).flip(-1).reshape(-1, 2)
                      for h, w in shapes])


def lattice_self(shapes, N, M, D, P, seed, weights=WEIGHTS, one_point=None):
    """locations = the query's own reference point + an offset of about 2 pixels (half of the samples) or about 9 pixels (the other half:
    beyond the near radius), rounded to sixteenths; `one_point`: every query samples within half a pixel of that point instead"""
    assert max(max(hw) for hw in shapes) <= 64
    g = torch.Generator().manual_seed(seed)
    S, L = sum(h * w for h, w in shapes), len(shapes)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    if one_point is None:
        ref = self_reference_points(shapes).view(1, S, 1, 1, 1, 2)
        px = torch.where(torch.rand(N, S, M, L, P, 1, generator=g) < 0.5, 2.0, 9.0)
    else:
        ref = torch.tensor(one_point).view(1, 1, 1, 1, 1, 2)
        px = 0.4
    off = torch.randn(N, S, M, L, P, 2, generator=g) * px / wh
    loc = (torch.round((ref + off) * 16) / 16).contiguous()
    attw = torch.tensor(weights)[torch.randint(0, len(weights), (N, S, M, L, P), generator=g)]
    value = torch.randint(-4, 5, (N, S, M, D), generator=g).float()
    gout = torch.randint(-1, 2, (N, S, M * D), generator=g).float()
    return dict(value=value, loc=loc, attw=attw, gout=gout)


def near_share(ops, shapes):
    """share of the in-map samples of a self-attention case within NEAR_PX pixels of their query's centre on the target level (fp64; the
    kernels decide in fp32, this only shows that both sides of the radius are populated)"""
    loc = ops["loc"].double()
    L = len(shapes)
    lq = torch.cat([torch.full((h * w,), i) for i, (h, w) in enumerate(shapes)])
    pos = torch.cat([torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij"), -1).flip(-1).reshape(-1, 2) for h, w in shapes]).double()
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)
    near = ins = 0
    for l in range(L):
        centre = (pos + 0.5) * (wh[l] / wh[lq]) - 0.5                       # (S, 2)
        xy = loc[:, :, :, l] * wh[l] - 0.5                                   # (N, S, M, P, 2)
        inside = ((xy > -1) & (xy < wh[l])).all(-1)
        nr = ((xy - centre.view(1, -1, 1, 1, 2)).abs() <= NEAR_PX).all(-1)
        near += int((inside & nr).sum())
        ins += int(inside.sum())
    return near / max(ins, 1)


# ------------------------------------------------------------------------------------------------ lattice MSDA: reference
def msda_ref(value, shapes, loc, attw, gout, absolute=False):
    """Multi-scale deformable attention sampling and its three gradients, written out in fp64 with the rule of the CUDA extension the
    kernel replaces: pixel coordinate x = loc_x * W - 0.5; a sample counts when y > -1 and x > -1 and y < H and x < W; its cell is
    floor(x), floor(y); a corner counts when it is in range; d / dx comes from lx = x - floor(x), times W (H) for the location.
    -> out (N, Lq, M * D), grad_value, grad_loc, grad_attw.
    absolute: the operands' magnitudes and every difference replaced by a sum -- each output is then the sum of the ABSOLUTE contributions
    to the element, the quantity that has to stay representable for the order of a sum not to matter."""
    value, loc, attw, gout = (t.double() for t in (value, loc, attw, gout))
    sgn = -1.0
    if absolute:
        value, attw, gout, sgn = value.abs(), attw.abs(), gout.abs(), 1.0
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = loc.shape
    g = gout.view(N, Lq, M, 1, D)
    out = value.new_zeros(N, Lq, M, D)
    gv, gl, ga = torch.zeros_like(value), torch.zeros_like(loc), torch.zeros_like(attw)
    n_idx, m_idx = torch.arange(N).view(N, 1, 1, 1), torch.arange(M).view(1, 1, M, 1)
    for l, ((H, W), start) in enumerate(zip(shapes, level_starts(shapes))):
        x, y, w = loc[:, :, :, l, :, 0] * W - 0.5, loc[:, :, :, l, :, 1] * H - 0.5, attw[:, :, :, l]          # (N, Lq, M, P)
        inside = (y > -1) & (x > -1) & (y < H) & (x < W)
        x0, y0 = torch.floor(x), torch.floor(y)
        lx, ly = x - x0, y - y0
        hx, hy = 1 - lx, 1 - ly
        d = {}
        for dy, wy in ((0, hy), (1, ly)):
            for dx, wx in ((0, hx), (1, lx)):
                xi, yi = (x0 + dx).long(), (y0 + dy).long()
                ok = (inside & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).double()
                idx = start + yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
                v = value[n_idx, idx, m_idx] * ok.unsqueeze(-1)                                               # (N, Lq, M, P, D)
                cw = wy * wx * ok
                out += ((w * cw).unsqueeze(-1) * v).sum(3)
                gv.index_put_((n_idx, idx, m_idx), (w * cw).unsqueeze(-1) * g, accumulate=True)
                d[dy, dx] = (v * g).sum(-1)
                ga[:, :, :, l] += cw * d[dy, dx]
        gl[:, :, :, l, :, 0] = w * (hy * (d[0, 1] + sgn * d[0, 0]) + ly * (d[1, 1] + sgn * d[1, 0])) * W
        gl[:, :, :, l, :, 1] = w * (hx * (d[1, 0] + sgn * d[0, 0]) + lx * (d[1, 1] + sgn * d[0, 1])) * H
    return out.reshape(N, Lq, M * D), gv, gl, ga


def sample_stats(loc, shapes):
    """shares of the samples: inside their level, with an exactly integer pixel coordinate, with a coordinate exactly -1, exactly W or H"""
    L = len(shapes)
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
    xy = loc.double() * wh - 0.5
    n = xy[..., 0].numel()
    return dict(inside=((xy > -1) & (xy < wh)).all(-1).sum().item() / n, integer=(xy == xy.round()).any(-1).sum().item() / n,
                minus_one=(xy == -1).any(-1).sum().item() / n, at_side=(xy == wh).any(-1).sum().item() / n, mask_minus_one=(xy == -1))


def check_lattice(ops, shapes, edges=True, mix=True):
    """the preconditions of the torch.equal tests, asserted on the reference side; -> the statistics.
    Exactness: with weights in quarters, bilinear fractions in sixteenths and integer values / gradients, a contribution to `out` or
    grad_value is a multiple of 2^-10, to grad_attw of 2^-8, to grad_loc of 2^-6 (before and after the integer factor W or H).  An fp32 sum
    of such terms is exact in any order while the sum of their magnitudes stays below 2^24 units: 2^14, 2^16 and 2^18.  (out is held to the
    2^14 of grad_value.)
    mix: the sample population the MSDA cases are meant to have; edges: coordinates exactly at -1 and at W, where a sixteenth reaches them."""
    for k, t in ops.items():
        unit = {"value": 1, "loc": 16, "attw": 4, "gout": 1}[k]
        assert torch.equal(t * unit, (t * unit).round()), k
    a_out, a_gv, a_gl, a_ga = msda_ref(ops["value"], shapes, ops["loc"], ops["attw"], ops["gout"], absolute=True)
    assert a_gv.max().item() < 2 ** 14 and a_out.max().item() < 2 ** 14, (a_gv.max().item(), a_out.max().item())
    assert a_ga.max().item() < 2 ** 16 and a_gl.max().item() < 2 ** 18, (a_ga.max().item(), a_gl.max().item())
    st = sample_stats(ops["loc"], shapes)
    if mix:
        assert st["inside"] >= 0.5 and st["integer"] >= 0.05, st
    if edges and has_edges(shapes):
        assert st["minus_one"] >= 0.003 and st["at_side"] >= 0.003, st
    return st


def msda_seed(case):
    N, M, D, Lq, shapes, P = case
    return 7 * N + 100 * M + D + 1000 * Lq + P


@functools.lru_cache(maxsize=None)
def msda_case(i):
    """operands, fp64 reference and statistics of MSDA_CASES[i], computed once and left unchanged"""
    N, M, D, Lq, shapes, P = MSDA_CASES[i]
    ops = lattice_msda(N, M, D, Lq, shapes, P, msda_seed(MSDA_CASES[i]))
    st = check_lattice(ops, shapes)
    return ops, msda_ref(ops["value"], shapes, ops["loc"], ops["attw"], ops["gout"]), st


@functools.lru_cache(maxsize=None)
def self_case(name):
    pyr, N, M, D, P, weights, one_point = SELF_CASES[name]
    shapes = SELF_PYRAMIDS[pyr]
    ops = lattice_self(shapes, N, M, D, P, 31 + len(name) + 10 * len(shapes), weights, one_point)
    st = check_lattice(ops, shapes, edges=False, mix=False)
    return shapes, ops, msda_ref(ops["value"], shapes, ops["loc"], ops["attw"], ops["gout"]), st


def pile_count(ops, shapes, l, X, Y):
    """samples of image 0, head 0 whose 2 x 2 footprint on level l touches pixel (X, Y) (the gather walk lists them for that pixel's tile)"""
    H, W = shapes[l]
    x, y = ops["loc"][0, :, 0, l, :, 0].double() * W - 0.5, ops["loc"][0, :, 0, l, :, 1].double() * H - 0.5
    inside = (y > -1) & (x > -1) & (y < H) & (x < W)
    x0, y0 = torch.floor(x), torch.floor(y)
    return int((inside & (x0 <= X) & (x0 + 1 >= X) & (y0 <= Y) & (y0 + 1 >= Y)).sum())


def gather_tile_logs(shapes, P, limit):
    """log2 of the tile edge aldi_ms_deform_attn_backward_self gives every level for a list limit (msda_gather_list)"""
    S = sum(h * w for h, w in shapes)
    out = []
    for h, w in shapes:
        spp = S * P / (h * w)
        out.append(3 if spp * 81 <= limit else 2 if spp * 25 <= limit else 1 if spp * 9 <= limit else 0)
    return out


# ------------------------------------------------------------------------------------------------ fp64-matched: the rule
def tolerance(ref32, ref64, factor=8.0):
    """a kernel may be `factor` times as far from the fp64 truth as the same function in fp32 on the CPU, plus four ulps of the largest entry"""
    return factor * (ref32.double() - ref64).abs().max().item() + 4 * 2.0 ** -24 * ref64.abs().max().item()


def both(fn, *operands, **kw):
    """-> (fn in fp32, fn in fp64) on the same fp32 operands; tensors of other dtypes and non-tensors pass through"""
    def cast(dt):
        return [o.to(dt) if torch.is_tensor(o) and o.is_floating_point() else o for o in operands]
    return fn(*cast(torch.float32), **kw), fn(*cast(torch.float64), **kw)


# ------------------------------------------------------------------------------------------------ small attention
MHA_CASES = [(2, 300, 8, 32), (1, 1, 1, 16), (1, 64, 2, 64), (1, 65, 3, 32), (3, 127, 2, 16)]     # (B, Q, H, Dh)


def mha_operands(B, Q, H, Dh, seed, spread=1.0):
    """q, k, v, dO as (B, Q, H * Dh); spread: the scores q k^T / sqrt(Dh) reach about +-spread * 4"""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, Q, H * Dh, generator=g) for _ in range(4))
    return q * spread, k, v, do


def mha_ref(q, k, v, do, H, scale, keep=None):
    """softmax(scale q k^T) v per head with the keep / (1 - p) factors `keep` (B, H, Q, Q) on the normalised probabilities, and its
    backward.  q, k, v, do (B, Q, H * Dh) -> out, lse (B, H, Q), dq, dk, dv, delta (B, H, Q)"""
    B, Q, d = q.shape
    qh, kh, vh, gh = (t.view(B, Q, H, d // H).transpose(1, 2) for t in (q, k, v, do))
    qs = qh * scale
    s = qs @ kh.transpose(-1, -2)
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    pk = p if keep is None else p * keep.to(p.dtype)
    out = pk @ vh
    delta = (gh * out).sum(-1)
    dv = pk.transpose(-1, -2) @ gh
    dp = gh @ vh.transpose(-1, -2)
    if keep is not None:
        dp = dp * keep.to(p.dtype)
    ds = p * (dp - delta.unsqueeze(-1))
    dq, dk = (ds @ kh) * scale, ds.transpose(-1, -2) @ qs
    back = lambda t: t.transpose(1, 2).reshape(B, Q, d)
    return dict(out=back(out), lse=lse, dq=back(dq), dk=back(dk), dv=back(dv), delta=delta)


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_CASES = [(2, 1961, 256, 32), (1, 1, 32, 32), (1, 256, 8, 2), (3, 257, 64, 4), (2, 700, 24, 4), (1, 5, 4096, 32), (2, 8400, 256, 32)]   # (N, HW, C, G)
GN_EPS = 1e-5


def gn_operands(N, HW, C, G, seed, offset=1.0, std=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, HW, C, generator=g) * std + offset
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    gy = torch.randn(N, HW, C, generator=g)
    dgamma0, dbeta0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, gamma, beta, gy, dgamma0, dbeta0


def gn_ref(x, gamma, beta, gy, dgamma0, dbeta0, G, eps=GN_EPS):
    """x, gy (N, HW, C) -> y, mean, rstd (N, G), dx, dgamma = dgamma0 + ..., dbeta = dbeta0 + ...; two-pass statistics"""
    N, HW, C = x.shape
    grp = lambda t: t.view(N, HW, G, C // G).permute(0, 2, 1, 3).reshape(N, G, -1)          # a group's elements contiguous: torch sums them pairwise
    ungrp = lambda t: t.view(N, G, HW, C // G).permute(0, 2, 1, 3).reshape(N, HW, C)
    xg = grp(x)
    mean = xg.mean(-1, keepdim=True)
    var = ((xg - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = ungrp((xg - mean) * rstd)
    y = xh * gamma + beta
    gg = grp(gy * gamma)
    a, b = gg.mean(-1, keepdim=True), (gg * grp(xh)).mean(-1, keepdim=True)
    dx = ungrp(rstd * (gg - a - grp(xh) * b))
    dgamma = dgamma0 + (gy * xh).reshape(-1, C).sum(0)
    dbeta = dbeta0 + gy.reshape(-1, C).sum(0)
    return dict(y=y, mean=mean.view(N, G), rstd=rstd.view(N, G), dx=dx, dgamma=dgamma, dbeta=dbeta)


def gn_torch(x, gamma, beta, gy, dgamma0, dbeta0, G, eps=GN_EPS):
    """the same outputs from torch's own group_norm (native_group_norm for the statistics, autograd for the backward), in x's dtype"""
    N, HW, C = x.shape
    xn = x.permute(0, 2, 1).reshape(N, C, HW, 1).contiguous().requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y, mean, rstd = torch.native_group_norm(xn, gm, bt, N, C, HW, G, eps)
    y.backward(gy.permute(0, 2, 1).reshape(N, C, HW, 1))
    to_nhwc = lambda t: t.detach().reshape(N, C, HW).permute(0, 2, 1).contiguous()
    return dict(y=to_nhwc(y), mean=mean.detach().view(N, G), rstd=rstd.detach().view(N, G), dx=to_nhwc(xn.grad), dgamma=dgamma0 + gm.grad, dbeta=dbeta0 + bt.grad)


# ------------------------------------------------------------------------------------------------ the sampling glue
PREPARE_CASES = [(600, 8, 4, 4), (1, 1, 1, 1), (257, 3, 5, 3)]           # (T, M, L, P)
PREPARE_SHAPES = ((25, 42), (13, 21), (7, 11), (4, 6), (2, 3))


def prepare_operands(T, M, L, P, seed, logit_span=1.0):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(T, M * L * P * 3, generator=g)
    raw[:, : M * L * P * 2] *= 3                                         # offsets of a few pixels
    raw[:, M * L * P * 2:] *= logit_span
    ref = torch.rand(T, L, 2, generator=g)
    g_loc, g_aw = torch.randn(T, M, L, P, 2, generator=g), torch.randn(T, M, L, P, generator=g)
    return raw, ref, g_loc, g_aw


def prepare_ref(raw, ref, g_loc, g_aw, shapes, M, L, P):
    """raw (T, M * L * P * 3) = the offset linear's outputs (M, L, P, 2) then the weight linear's (M, L * P); ref (T, L, 2)
    -> loc = ref + offset / (W_l, H_l), aw = softmax over (level, point), and the backward: g_raw, g_ref = sum over heads and points"""
    T = raw.shape[0]
    LP = L * P
    off, lg = raw[:, : M * LP * 2].view(T, M, L, P, 2), raw[:, M * LP * 2:].view(T, M, LP)
    wh = torch.tensor([[w, h] for h, w in shapes[:L]], dtype=raw.dtype).view(1, 1, L, 1, 2)
    loc = ref.view(T, 1, L, 1, 2) + off / wh
    aw = torch.softmax(lg, -1)
    ga = g_aw.view(T, M, LP)
    g_lg = aw * (ga - (aw * ga).sum(-1, keepdim=True))
    g_raw = torch.cat([(g_loc / wh).reshape(T, -1), g_lg.reshape(T, -1)], 1)
    return dict(loc=loc, aw=aw.view(T, M, L, P), g_raw=g_raw, g_ref=g_loc.sum((1, 3)))


# ------------------------------------------------------------------------------------------------ the box head's last step
def box_operands(R, refs, seed):
    """reference coordinates exactly 0 and 1, below 0 and above 1, inside (0, 1e-5) and (1 - 1e-5, 1), every one at least 1e-6 away from
    the two kinks 1e-5 and 1 - 1e-5 (where the fp32 and fp64 clamps may switch on different sides)"""
    g = torch.Generator().manual_seed(seed)
    special = torch.tensor([0.0, 1.0, -0.25, 1.5, 3e-6, 8e-6, 1 - 3e-6, 1 - 8e-6, 1.2e-5, 1 - 1.2e-5, 0.5, 1e-3])
    ref = torch.rand(refs, 2, generator=g)
    pick = torch.randint(0, 3 * len(special), (refs, 2), generator=g)       # a third of the coordinates are special
    ref = torch.where(pick < len(special), special[pick.clamp(max=len(special) - 1)], ref)
    if refs >= len(special):
        ref[: len(special), 0] = special
        ref[: len(special), 1] = special.flip(0)
    else:
        ref[0, 0], ref[0, 1] = 0.0, 1 - 3e-6
    for kink in (1e-5, 1 - 1e-5):
        assert ((ref.double() - kink).abs() >= 1e-6).all()
    t = torch.randn(R, 4, generator=g) * 2
    return t, ref, torch.randn(R, 4, generator=g), torch.randn(refs, 2, generator=g)


def box_ref(t, ref, g_boxes, g_ref0, eps=EPS_BOX):
    """boxes = sigmoid(t + (logit(ref[r % refs]), 0, 0)) with the clamps of inverse_sigmoid; g_t, g_ref = g_ref0 + the rows' gradients"""
    R, refs = t.shape[0], ref.shape[0]
    row = torch.arange(R) % refs
    u = ref.clamp(0, 1)
    lo = torch.log(u.clamp(min=eps) / (1 - u).clamp(min=eps))
    x = torch.cat([t[:, :2] + lo[row], t[:, 2:]], 1)
    boxes = torch.sigmoid(x)
    g_t = g_boxes * boxes * (1 - boxes)
    one, zero = torch.ones_like(ref), torch.zeros_like(ref)
    d = torch.where(u > eps, one / u.clamp(min=eps), zero) + torch.where(1 - u > eps, one / (1 - u).clamp(min=eps), zero)
    d = torch.where((ref >= 0) & (ref <= 1), d, zero)
    g_ref = g_ref0 + torch.zeros_like(ref).index_add_(0, row, g_t[:, :2]) * d
    return dict(boxes=boxes, g_t=g_t, g_ref=g_ref, g_ref_plain=g_ref - g_ref0)


# ------------------------------------------------------------------------------------------------ the set criterion at saturated logits
def criterion_operands(seed, Ld=2, B=3, Nq=40, K=7):
    g = torch.Generator().manual_seed(seed)
    levels = torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0])
    logits = levels[torch.randint(0, len(levels), (Ld, B, Nq, K), generator=g)]
    boxes = torch.cat([torch.rand(Ld, B, Nq, 2, generator=g) * 0.6 + 0.2, torch.rand(Ld, B, Nq, 2, generator=g) * 0.3 + 0.05], -1)
    targets = [{"labels": torch.randint(0, K, (n,), generator=g), "boxes": torch.cat([torch.rand(n, 2, generator=g) * 0.6 + 0.2, torch.rand(n, 2, generator=g) * 0.3 + 0.05], -1)}
               for n in (5, 0, 3)]
    return logits, boxes, targets


def criterion_ref(logits, boxes, targets, indices, weights=(2.0, 5.0, 2.0)):
    """oracle.deformable_detr.criterion with the assignment given (`indices[l]`: the oracle's pairs of layer l, so that the fp32 and the
    fp64 run and the kernel score the same pairs) -> weighted losses (Ld, 3), d(total) / d(logits), d(total) / d(boxes), in logits' dtype"""
    from oracle import deformable_detr as D
    lg, bx = logits.clone().requires_grad_(True), boxes.clone().requires_grad_(True)
    tg = [{"labels": t["labels"], "boxes": t["boxes"].to(logits.dtype)} for t in targets]
    rows, total = [], 0.0
    for l in range(logits.shape[0]):
        d, _ = D.set_losses(lg[l], bx[l], tg, indices=indices[l])
        rows.append(torch.stack([w * d[k] for k, w in zip(("loss_ce", "loss_bbox", "loss_giou"), weights)]))
        total = total + rows[-1].sum()
    total.backward()
    return dict(losses=torch.stack(rows).detach(), g_logits=lg.grad, g_boxes=bx.grad)

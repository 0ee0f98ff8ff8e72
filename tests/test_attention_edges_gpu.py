"""Attention kernels (aldi_amd/csrc/attn.hip) at the masking edges, against operand-matched fp64 references.

The reference is written out here (no library attention):

    bias[q,k] = q . Rh[qh - kh + gh - 1] + q . Rw[qw - kw + gw - 1]
    S = (q/8) . k + bias        P = softmax(S)        O = P v        lse = logsumexp(S)

The kernels round the tables and the bias columns of Q' to bf16, so a comparison with the plain reference needs a tolerance
that hides real faults.  The staged checks instead read the workspaces of `vit_ops.Attention` back: the prep kernels are
checked exactly, and every MFMA kernel is checked against fp64 on the operands the device itself produced, with a PER-ELEMENT
envelope that covers only that kernel's own roundings (U8 = 2^-8 is the bf16 unit roundoff, E32 = 2^-24 the fp32 one).  One
end-to-end assertion per shape against the unrounded reference keeps the staged checks tied to the real operation.

The generators and the reference run on any device; tests/test_attention_reference_cpu.py checks them without a GPU.
DESIGN.md ("Attention test bounds") records the measured worst ratios; every `ATTN_EDGES` line printed here feeds that table."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = 2.0 ** -8         # bf16: 8 significand bits, round to nearest => relative error <= 2^-8
E32 = 2.0 ** -24

# envelope constants: the roundings counted in the kernels
# O: 3 * 2^-9 * (P.|v|) + 2^-9 * |O|, the form this bound was specified in.  It is a worst-case bound: P -> bf16 costs <= U8 (P.|v|), the bf16 store
# <= U8 |O|, and U8 (P.|v|) + U8 |O| <= 1.5 U8 (P.|v|) + 0.5 U8 |O| because |O| <= P.|v|.
C_O_P = 3 * 2.0 ** -9
C_O_OUT = 2.0 ** -9
C_BWD = 2.125 * U8     # dS (or P) -> bf16 for the second MFMA, result -> bf16 (U8 |result| <= U8 |dS|.|K'|); the eighth covers __expf and
                       # the fp32 accumulation of S: E32 * (sum|Q'||K'| + 2|S - lse| + 4) <= U8 / 8 for sum|Q'||K'| < 8000
C_DQ = 1.125 * U8      # attn_rel_dq_kernel: fp32 accumulation of bf16 operands, ONE bf16 store
C_DELTA = 8 * E32      # attn_bwd_prep_kernel: exact bf16 products, 6-level butterfly sum in fp32 (+2 for the operands' order)
# lse is fp32 from matched operands.  Its error in units of E32: the final m + log(l) rounds at |lse|; the fp32 accumulation of S
# rounds at sum|Q'||K'| once per 32-wide MFMA step; __expf (v_exp_f32 of x * log2e) and __logf contribute a few ulp at magnitude
# <= 17 (terms below 2^-24 of the row maximum do not reach the sum), and the L-term sum adds <= (16 + tiles) roundings of a value
# whose log is taken.  Unit per row: E32 * (64 + max_k sum_d |Q'||K'|); the bound is LSE_C units = 4 x the measured worst ratio.
LSE_C = 2.7          # measured worst 0.664 units (selector, 9 x 25, winning logit ~128); random data 0.26 units = 1.3e-6 absolute

# nB, gh, gw, heads, rel, tiled, Dq, arm
SHAPES = [
    (2, 15, 15, 2, False, False, 64, "linear 4-wave, L=225, 31 masked slots"),
    (1, 16, 16, 3, False, False, 64, "linear 4-wave, L=Lp=256"),
    (1, 19, 23, 1, False, False, 64, "linear 4-wave, four query blocks, ragged"),
    (2, 3, 60, 2, True, False, 128, "linear NKS=4"),
    (1, 2, 100, 2, True, False, 192, "linear NKS=6"),
    (2, 14, 16, 2, True, False, 96, "L=224: last size of the 7-wave arm"),
    (2, 15, 15, 2, True, True, 96, "L=225: smallest tiled grid, 7 of 8 rows/cols"),
    (1, 9, 25, 2, True, True, 128, "tiled, one valid row / column in the last blocks"),
    (3, 1, 1, 1, True, False, 96, "single token"),
    (2, 1, 3, 2, True, False, 96, "three tokens"),
    (1, 8, 184, 1, True, True, 256, "tiled at Dq=256 (8 x 128 only reaches 224)"),
    (1, 2, 113, 1, True, True, 192, "tiled, thin: tile-major k^T larger than Dq x Lp"),
    (1, 1, 190, 1, True, False, 256, "linear NKS=8, LDS > 64 KB"),
    (1, 1, 191, 1, True, False, 256, "linear NKS=8, LDS > 64 KB, odd"),
]
IDS = ["%dx%dx%dx%d%s" % (s[0], s[1], s[2], s[3], "" if s[4] else "-norel") for s in SHAPES]


def layout(gh, gw, rel):
    """The layout rules of attn.hip (layout_of), restated; the GPU tests assert that the library agrees."""
    L = gh * gw
    Lp = (L + 63) // 64 * 64
    tiled = bool(rel) and L > 7 * 32
    ghp, gwp = (gh + 7) // 8 * 8, (gw + 7) // 8 * 8
    wofs = ghp if tiled else gh
    need = 64 + wofs + (gwp if tiled else gw) if rel else 64
    ntw = gwp // 8
    nt2 = (ghp // 8) * ntw
    return dict(L=L, Lp=Lp, tiled=tiled, ghp=ghp, gwp=gwp, wofs=wofs, Dq=(need + 31) // 32 * 32, ntw=ntw, nt2=nt2,
                vt_cols=nt2 * 64 if tiled and nt2 * 64 > Lp else Lp)


def padded_slots(shape):
    lay = layout(shape[1], shape[2], shape[4])
    return (lay["ghp"] * lay["gwp"] if lay["tiled"] else lay["Lp"]) - lay["L"]


PADDED = [s for s in SHAPES if padded_slots(s) > 0]
PADDED_IDS = [i for s, i in zip(SHAPES, IDS) if padded_slots(s) > 0]


# ------------------------------------------------------------------------------------------------ fp64 reference
def split_heads(x, nB, L, heads):
    """[nB*L, n*heads*64] -> n tensors [nB*heads, L, 64]"""
    n = x.shape[1] // (heads * 64)
    t = x.reshape(nB, L, n, heads, 64).permute(2, 0, 3, 1, 4).reshape(n, nB * heads, L, 64)
    return t.unbind(0) if n > 1 else t[0]


def merge_heads(ts, nB, L, heads):
    """n tensors [nB*heads, L, 64] -> [nB*L, n*heads*64]"""
    t = torch.stack(list(ts)).reshape(len(ts), nB, heads, L, 64).permute(1, 3, 0, 2, 4)
    return t.reshape(nB * L, len(ts) * heads * 64)


def rel_index(g, device):
    a = torch.arange(g, device=device)
    return a[:, None] - a[None, :] + g - 1          # [q coordinate, k coordinate]


def rel_bias_parts(q, rel_h, rel_w, gh, gw):
    """q [BH, L, 64] -> (q . Rh[qh-kh+gh-1]) [BH, gh, gw, kh] and (q . Rw[qw-kw+gw-1]) [BH, gh, gw, kw]"""
    qg = q.reshape(q.shape[0], gh, gw, 64)
    bh = torch.einsum("bhwc,hkc->bhwk", qg, rel_h[rel_index(gh, q.device)])
    bw = torch.einsum("bhwc,wkc->bhwk", qg, rel_w[rel_index(gw, q.device)])
    return bh, bw


def attention_ref(qkv, rel_h, rel_w, nB, gh, gw, heads):
    """fp64 attention with decomposed relative positions -> O [nB*L, heads*64], lse [nB*heads, L], S [nB*heads, L, L]"""
    L = gh * gw
    q, k, v = split_heads(qkv.double(), nB, L, heads)
    S = (q * 0.125) @ k.transpose(1, 2)
    if rel_h is not None:
        bh, bw = rel_bias_parts(q, rel_h.double(), rel_w.double(), gh, gw)
        S = S + (bh[..., :, None] + bw[..., None, :]).reshape(S.shape)
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    return merge_heads([P @ v], nB, L, heads), lse, S


# ------------------------------------------------------------------------------------------------ input generators (CPU, seeded)
def _tables(g, gh, gw, scale):
    return ((torch.randn(2 * gh - 1, 64, generator=g) * scale).bfloat16().float(),
            (torch.randn(2 * gw - 1, 64, generator=g) * scale).bfloat16().float())


def gen_random(shape, seed=0):
    """The data of test_attention_fwd_bwd: qkv ~ 1.5 N(0,1) in bf16, fp32 tables ~ 0.1 N(0,1) (NOT bf16-representable)."""
    nB, gh, gw, heads, rel = shape[:5]
    g = torch.Generator().manual_seed(1000 + seed)
    L = gh * gw
    qkv = (torch.randn(nB * L, 3 * heads * 64, generator=g) * 1.5).bfloat16()
    rel_h = torch.randn(2 * gh - 1, 64, generator=g) * 0.1 if rel else None
    rel_w = torch.randn(2 * gw - 1, 64, generator=g) * 0.1 if rel else None
    dO = torch.randn(nB * L, heads * 64, generator=g).bfloat16()
    return qkv, rel_h, rel_w, dO


def gen_mask_leak(shape, seed=0):
    """q = +18 u + noise, k = -18 u + noise with u = (1/8, ..., 1/8): every real logit is about -40.5 (bias |.| < 12 included), so one
    leaked slot (k = v = 0: logit 0) takes all the mass.  v = 1 +- 0.375: a leak drives O from about 1 to 0.  All values are bf16 numbers."""
    nB, gh, gw, heads, rel = shape[:5]
    g = torch.Generator().manual_seed(2000 + seed)
    BH, L = nB * heads, gh * gw
    noise = lambda: torch.randint(-4, 5, (BH, L, 64), generator=g).float() / 64
    q, k = 2.25 + noise(), -2.25 + noise()
    v = 1 + torch.randint(-6, 7, (BH, L, 64), generator=g).float() / 16
    qkv = merge_heads([q, k, v], nB, L, heads)
    assert torch.equal(qkv.bfloat16().float(), qkv)
    rel_h, rel_w = _tables(g, gh, gw, 0.05) if rel else (None, None)
    dO = torch.randn(nB * L, heads * 64, generator=g).bfloat16()
    return qkv.bfloat16(), rel_h, rel_w, dO


def _hadamard(n):
    h = torch.ones(1, 1)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def selector_modes(shape):
    return ("qk", "bias+", "bias-") if shape[4] else ("qk",)


def gen_selector(shape, mode, seed=0):
    """Every query gets one key that wins by >= 40 in logit -> qkv, tables, winner [BH, L] (-1: no single winner for that query).

    "qk": key j carries the code 4 * [h(j // 64) | h(j % 64)], h = the 64 rows of +-Hadamard(32) (pairwise products <= 0); query i
    carries the code of key perm[i].  Winner 128, every other key <= 64; small random tables move that by a few units.
    "bias+" / "bias-": q = 8 e0 for every query, k[0] = 0 (q.k = 0), the tables are zero but for an 8 at ONE relative offset each, so the
    key displaced by (dh, dw) from the query collects 64 + 64, a key matching one offset 64, any other 0."""
    nB, gh, gw, heads, rel = shape[:5]
    g = torch.Generator().manual_seed(3000 + seed)
    BH, L = nB * heads, gh * gw
    v = torch.randn(BH, L, 64, generator=g).bfloat16().float()
    if mode == "qk":
        assert L <= 4096
        h32 = _hadamard(32)
        half = torch.cat([h32, -h32], 0)                                  # 64 codewords of length 32
        j = torch.arange(L)
        code = 4 * torch.cat([half[j // 64], half[j % 64]], 1)            # [L, 64]
        winner = torch.stack([torch.randperm(L, generator=g) for _ in range(BH)])
        k = code[None].expand(BH, L, 64)
        q = code[winner]
        rel_h, rel_w = _tables(g, gh, gw, 0.01) if rel else (None, None)
    else:
        dh, dw = (1, -1) if mode == "bias+" else (-2, 3)
        dh = max(-(gh - 1), min(gh - 1, dh))
        dw = max(-(gw - 1), min(gw - 1, dw))
        q = torch.zeros(BH, L, 64)
        q[..., 0] = 8
        k = torch.randn(BH, L, 64, generator=g).bfloat16().float()
        k[..., 0] = 0
        rel_h, rel_w = torch.zeros(2 * gh - 1, 64), torch.zeros(2 * gw - 1, 64)
        rel_h[gh - 1 + dh, 0] = 8
        rel_w[gw - 1 + dw, 0] = 8
        t = torch.arange(L)
        kh, kw = t // gw - dh, t % gw - dw
        ok = (kh >= 0) & (kh < gh) & (kw >= 0) & (kw < gw)
        winner = torch.where(ok, kh * gw + kw, torch.full_like(t, -1))[None].expand(BH, L).contiguous()
    return merge_heads([q, k, v], nB, L, heads).bfloat16(), rel_h, rel_w, winner


def selector_margin(S, winner):
    """smallest (winning logit - best other logit) over the queries that have a winner"""
    has = winner >= 0
    w = winner.clamp_min(0)
    win = S.gather(2, w[..., None])[..., 0]
    other = S.scatter(2, w[..., None], float("-inf")).max(dim=2).values
    return (win - other)[has].min().item(), win


# ------------------------------------------------------------------------------------------------ staged device checks
def report(tag, name, value):
    print("ATTN_EDGES %-18s %-10s %.4g" % (tag, name, value))


def bf16_ord(x):
    """bf16 -> integer that is monotone in the value (+-0 -> 0): neighbours differ by 1"""
    b = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = b & 0x7FFF
    return torch.where(b >= 0x8000, -mag, mag)


def worst_ratio(got, ref, env):
    """largest |got - ref| / env over the elements that differ at all"""
    err = (got - ref).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / env.clamp_min(1e-300)).max().item()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def kprime(k, shape, lay):
    """K' = [k | onehot(kh) | onehot(kw)] [BH, L, Dq] in k's dtype"""
    gh, gw, rel = shape[1], shape[2], shape[4]
    BH, L = k.shape[0], k.shape[1]
    Kp = torch.zeros(BH, L, lay["Dq"], dtype=k.dtype, device=k.device)
    Kp[..., :64] = k
    if rel:
        t = torch.arange(L, device=k.device)
        Kp[:, t, 64 + t // gw] = 1
        Kp[:, t, 64 + lay["wofs"] + t % gw] = 1
    return Kp


def live_columns(shape, lay, device):
    """columns of Q' / dQ' that may be non-zero: q, the gh valid kh columns, the gw valid kw columns"""
    m = torch.zeros(lay["Dq"], dtype=torch.bool, device=device)
    m[:64] = True
    if shape[4]:
        m[64:64 + shape[1]] = True
        m[64 + lay["wofs"]:64 + lay["wofs"] + shape[2]] = True
    return m


def pad_T(x, Lp):
    """[BH, L, D] -> [BH, D, Lp], zero-padded"""
    out = torch.zeros(x.shape[0], x.shape[2], Lp, dtype=x.dtype, device=x.device)
    out[..., :x.shape[1]] = x.transpose(1, 2)
    return out


def tile_major(x, shape, lay):
    """[BH, L, 64] -> [BH, nt2, 64 d, 64 slots]: rows gathered at slot_token, zero where the slot is outside the grid"""
    gh, gw = shape[1], shape[2]
    kt, s = torch.arange(lay["nt2"], device=x.device)[:, None], torch.arange(64, device=x.device)[None, :]
    r, c = 8 * (kt // lay["ntw"]) + (s >> 3), 8 * (kt % lay["ntw"]) + (s & 7)
    ok = ((r < gh) & (c < gw)).reshape(-1)
    tok = torch.where(ok, (r * gw + c).reshape(-1), torch.zeros_like(ok, dtype=torch.long))
    t = torch.where(ok[None, :, None], x[:, tok], torch.zeros((), dtype=x.dtype, device=x.device))
    return t.reshape(x.shape[0], lay["nt2"], 64, 64).transpose(2, 3)


def make_att(shape):
    from aldi_amd import vit_ops as V
    nB, gh, gw, heads, rel, tiled, Dq = shape[:7]
    att = V.Attention(nB, gh, gw, heads, DEV, rel=rel)
    lay = layout(gh, gw, rel)
    assert (att.tiled, att.Dq) == (tiled, Dq) == (lay["tiled"], lay["Dq"]), (att.tiled, att.Dq)
    assert att.VT.shape[2] == lay["vt_cols"] and att.Lp == lay["Lp"]
    BH = nB * heads
    if tiled:       # the tile-major k^T / V^T need 64 x 64 elements per 8x8 key block
        assert att.KpT.numel() >= BH * lay["nt2"] * 4096 and att.VT.numel() >= BH * lay["nt2"] * 4096
    return att, lay


def check_prep(att, lay, shape, qkv, rel_h, rel_w, tag):
    nB, gh, gw, heads, rel = shape[:5]
    BH, L, Lp, wofs = nB * heads, gh * gw, lay["Lp"], lay["wofs"]
    q, k, v = split_heads(qkv, nB, L, heads)
    Qp = att.Qp
    assert same_bits(Qp[..., :64], (q.float() * 0.125).bfloat16())
    live = live_columns(shape, lay, qkv.device)
    assert (Qp[..., ~live].contiguous().view(torch.int16) == 0).all(), "Q' columns outside q / valid kh / valid kw must be +0"
    if rel:
        th, tw = rel_h.bfloat16().double(), rel_w.bfloat16().double()
        bh, bw = rel_bias_parts(q.double(), th, tw, gh, gw)
        ah, aw = rel_bias_parts(q.double().abs(), th.abs(), tw.abs(), gh, gw)
        exact = torch.cat([bh.reshape(BH, L, gh), bw.reshape(BH, L, gw)], 2)
        # the kernel's fp32 value e (two chained 32-term MFMA steps) obeys |e - exact| <= 4 E32 sum|q||R|, and the column is bf16(e)
        slack = 4 * E32 * torch.cat([ah.reshape(BH, L, gh), aw.reshape(BH, L, gw)], 2)
        got = bf16_ord(torch.cat([Qp[..., 64:64 + gh], Qp[..., 64 + wofs:64 + wofs + gw]], 2))
        want = bf16_ord(exact.float().bfloat16())
        lo, hi = bf16_ord((exact - slack).float().bfloat16()), bf16_ord((exact + slack).float().bfloat16())
        d = (got - want).abs()
        share = (d != 0).double().mean().item()
        report(tag, "bias_ulp", share)
        report(tag, "bias_maxulp", d.max().item())
        # "within one bf16 ulp of bf16(exact)", stated so that it also holds where the dot product cancels to almost nothing (there
        # the fp32 accumulation error exceeds an ulp of the tiny result): the column must be the rounding of a value in exact +- slack.
        # For |exact| >> slack that interval contains a single bf16 number, or two next to a rounding boundary.
        assert ((got >= lo) & (got <= hi)).all(), "bias column is not bf16(fp64 dot) to fp32 accumulation: wrong table row?"
        assert (d[exact.abs() >= 2 ** 10 * slack] <= 1).all()
        assert share < 1e-3
    assert same_bits(att.QsT, pad_T(Qp[..., :64], Lp))
    if not lay["tiled"]:
        assert same_bits(att.Kp, kprime(k, shape, lay))
        assert same_bits(att.KpT, pad_T(att.Kp, Lp))
        assert same_bits(att.VT, pad_T(v, Lp))
    else:
        n = lay["nt2"] * 4096
        assert lay["vt_cols"] * 64 == n             # the tile-major V^T fills VT exactly: nothing beyond the last tile
        assert same_bits(att.KpT.reshape(BH, -1)[:, :n].reshape(BH, lay["nt2"], 64, 64), tile_major(k, shape, lay))
        assert same_bits(att.VT.reshape(BH, -1)[:, :n].reshape(BH, lay["nt2"], 64, 64), tile_major(v, shape, lay))


def matched_scores(att, lay, shape, qkv):
    """fp64 S = Q' K'^T on the device's own Q' (K' from Kp on the linear path, rebuilt on the tiled one) + the lse unit per row"""
    nB, gh, gw, heads = shape[:4]
    q, k, v = split_heads(qkv, nB, gh * gw, heads)
    Kp = (kprime(k, shape, lay) if lay["tiled"] else att.Kp).double()
    Qp = att.Qp.double()
    S = Qp @ Kp.transpose(1, 2)
    unit = E32 * (64 + (Qp.abs() @ Kp.abs().transpose(1, 2)).max(dim=2).values)
    return S, Kp, Qp, v.double(), unit


def check_forward(att, lay, shape, qkv, O, lse, tag):
    nB, gh, gw, heads = shape[:4]
    S, Kp, Qp, v, unit = matched_scores(att, lay, shape, qkv)
    lse_ref = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse_ref[..., None])
    O_ref = P @ v
    env = C_O_P * (P @ v.abs()) + C_O_OUT * O_ref.abs()
    Od = split_heads(O, nB, gh * gw, heads).double()
    assert torch.isfinite(Od).all() and torch.isfinite(lse).all()
    rO = worst_ratio(Od, O_ref, env)
    e_lse = (lse.double() - lse_ref).abs()
    rl = worst_ratio(lse.double(), lse_ref, unit)
    report(tag, "O", rO)
    report(tag, "lse", rl)
    report(tag, "lse_abs", e_lse.max().item())
    assert rO <= 1.0, rO
    assert rl <= LSE_C, rl
    return lse_ref, O_ref


def check_backward(att, lay, shape, qkv, rel_h, rel_w, O, lse, dO, dqkv, drel0, drel, tag):
    nB, gh, gw, heads, rel = shape[:5]
    BH, L, wofs = nB * heads, gh * gw, lay["wofs"]
    S, Kp, Qp, v, _ = matched_scores(att, lay, shape, qkv)
    Oh, dOh = split_heads(O, nB, L, heads), split_heads(dO, nB, L, heads)
    # exact part: delta (exact products, fp32 butterfly) and the zero-padded transpose of dO
    prod = Oh.double() * dOh.double()
    r = worst_ratio(att.delta.double(), prod.sum(-1), C_DELTA * prod.abs().sum(-1))
    report(tag, "delta", r)
    assert r <= 1.0, r
    assert same_bits(att.dOT, pad_T(dOh, lay["Lp"]))
    # dS from the kernel's own lse and delta.  Roundings in attn_bwd_dq(2d)_kernel / attn_bwd_dkv(2d)_kernel: dS (resp. P) -> bf16
    # for the second MFMA, the result -> bf16 (<= U8 |result| <= U8 |dS|.|K'|), P from __expf of an fp32 S: C_BWD.  dP - delta is a
    # difference of two fp32 values: absolute error 4 E32 (|dO|.|v| + |delta|) (two MFMA steps, the delta sum, the subtraction), x P.
    dOd, delta = dOh.double(), att.delta.double()[..., None]
    P = torch.exp(S - lse.double()[..., None])
    dS = P * (dOd @ v.transpose(1, 2) - delta)
    env_dS = C_BWD * dS.abs() + P * (4 * E32) * (dOd.abs() @ v.abs().transpose(1, 2) + delta.abs())
    dq_d, dk_d, dv_d = (t.double() for t in split_heads(dqkv, nB, L, heads))
    dQ = att.dQp.double()
    assert torch.isfinite(dQ).all() and torch.isfinite(dqkv.float()).all()
    live = live_columns(shape, lay, qkv.device)
    assert (att.dQp[..., ~live].contiguous().view(torch.int16) == 0).all(), "dQ' columns without a key coordinate must be +0"
    Qs = Qp[..., :64]
    for name, got, ref, env in (("dQp", dQ, dS @ Kp, env_dS @ Kp.abs()),
                                ("dk", dk_d, dS.transpose(1, 2) @ Qs, env_dS.transpose(1, 2) @ Qs.abs()),
                                ("dv", dv_d, P.transpose(1, 2) @ dOd, C_BWD * (P.transpose(1, 2) @ dOd.abs()))):
        r = worst_ratio(got, ref, env)
        report(tag, name, r)
        assert r <= 1.0, (name, r)
        assert not ((got == 0) & (ref.abs() > env)).any(), name + " is zero where the reference is not"
    # dq and the table gradients from the device's own dQ': dq = dQ'[:, :64] / 8 + sum dbias . bf16(table),  drel = sum_q dbias . q
    q = split_heads(qkv, nB, L, heads)[0].double()
    dq_ref, E = dQ[..., :64] * 0.125, dQ[..., :64].abs() * 0.125
    if rel:
        th, tw = rel_h.bfloat16().double()[rel_index(gh, qkv.device)], rel_w.bfloat16().double()[rel_index(gw, qkv.device)]
        dbh = dQ[..., 64:64 + gh].reshape(BH, gh, gw, gh)
        dbw = dQ[..., 64 + wofs:64 + wofs + gw].reshape(BH, gh, gw, gw)
        dq_ref = dq_ref + (torch.einsum("bhwk,hkc->bhwc", dbh, th) + torch.einsum("bhwk,wkc->bhwc", dbw, tw)).reshape(BH, L, 64)
        E = E + (torch.einsum("bhwk,hkc->bhwc", dbh.abs(), th.abs()) + torch.einsum("bhwk,wkc->bhwc", dbw.abs(), tw.abs())).reshape(BH, L, 64)
    r = worst_ratio(dq_d, dq_ref, C_DQ * E)
    report(tag, "dq", r)
    assert r <= 1.0, r
    if rel:
        # attn_rel_dtab_kernel: bf16 operands (q exactly: the 1/8 of (scale q)^T is undone in fp32), fp32 accumulation only.  Per output
        # element: 2 MFMA accumulations per 64-token tile (counted as 4 roundings each for the 32-term sum inside) and one atomic per
        # block, every one of them at a magnitude <= |start value| + sum |dbias||q|.
        qg = q.reshape(BH, gh, gw, 64)
        c_tab = E32 * (4 + 9 * BH * (lay["Lp"] // 64))
        for name, db, g, eq in (("drel_h", dbh, gh, "bhwk,bhwc->hkc"), ("drel_w", dbw, gw, "bhwk,bhwc->wkc")):
            idx = rel_index(g, qkv.device).reshape(-1)
            ref = drel0[name].double().index_add(0, idx, torch.einsum(eq, db, qg).reshape(-1, 64))
            env = c_tab * drel0[name].double().abs().index_add(0, idx, torch.einsum(eq, db.abs(), qg.abs()).reshape(-1, 64))
            r = worst_ratio(drel[name].double(), ref, env)
            report(tag, name, r)
            assert r <= 1.0, (name, r)


def drel_buffers(shape, fill):
    if not shape[4]:
        return dict(drel_h=None, drel_w=None)
    g = torch.Generator().manual_seed(7)
    mk = lambda n: (torch.randn(n, 64, generator=g) if fill else torch.zeros(n, 64)).to(DEV)
    return dict(drel_h=mk(2 * shape[1] - 1), drel_w=mk(2 * shape[2] - 1))


def run_device(shape, inputs, fill_drel=True):
    """forward + backward through a fresh Attention -> everything the checks read"""
    qkv, rel_h, rel_w, dO = (None if t is None else t.to(DEV) for t in inputs)
    att, lay = make_att(shape)
    O, lse = att.forward(qkv, rel_h, rel_w)
    drel0 = drel_buffers(shape, fill_drel)
    drel = {n: None if t is None else t.clone() for n, t in drel0.items()}
    dqkv = att.backward(qkv, rel_h, rel_w, O, lse, dO, drel["drel_h"], drel["drel_w"], prepared=True)
    torch.cuda.synchronize()
    return dict(att=att, lay=lay, qkv=qkv, rel_h=rel_h, rel_w=rel_w, dO=dO, O=O, lse=lse, dqkv=dqkv, drel0=drel0, drel=drel)


@functools.lru_cache(maxsize=None)
def random_run(i):
    return run_device(SHAPES[i], gen_random(SHAPES[i]))


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# ------------------------------------------------------------------------------------------------ tests: random data, staged
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_prep_operands(i):
    r = random_run(i)
    check_prep(r["att"], r["lay"], SHAPES[i], r["qkv"], r["rel_h"], r["rel_w"], IDS[i])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_forward_matched(i):
    r = random_run(i)
    check_forward(r["att"], r["lay"], SHAPES[i], r["qkv"], r["O"], r["lse"], IDS[i])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_backward_matched(i):
    """also: drel_h / drel_w start from random contents and must ACCUMULATE (the reference adds the start values)"""
    r = random_run(i)
    check_backward(r["att"], r["lay"], SHAPES[i], r["qkv"], r["rel_h"], r["rel_w"], r["O"], r["lse"], r["dO"], r["dqkv"], r["drel0"],
                   r["drel"], IDS[i])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_end_to_end(i):
    """the one assertion against the tensor maximum: pure fp64 reference, unrounded tables, the bounds of test_attention_fwd_bwd"""
    r, shape = random_run(i), SHAPES[i]
    nB, gh, gw, heads, rel = shape[:5]
    qr = r["qkv"].double().requires_grad_(True)
    rh = r["rel_h"].double().requires_grad_(True) if rel else None
    rw = r["rel_w"].double().requires_grad_(True) if rel else None
    O_ref, lse_ref, _ = attention_ref(qr, rh, rw, nB, gh, gw, heads)
    O_ref.backward(r["dO"].double())
    assert relerr(r["O"], O_ref) < 2e-2
    assert (r["lse"].double() - lse_ref).abs().max().item() < 5e-2
    third = heads * 64
    grads = [("dq", r["dqkv"][:, :third], qr.grad[:, :third]), ("dk", r["dqkv"][:, third:2 * third], qr.grad[:, third:2 * third]),
             ("dv", r["dqkv"][:, 2 * third:], qr.grad[:, 2 * third:])]
    if rel:
        grads += [(n, r["drel"][n] - r["drel0"][n], t.grad) for n, t in (("drel_h", rh), ("drel_w", rw))]
    # Gradients that are identically zero have no maximum to relate an error to: with one key P = 1 and dS = 0 (dq, dk), and a
    # table with a single row collects sum_k dS[q,k] = 0 (drel_h for gh = 1, drel_w for gw = 1).  The device leaves rounding
    # residue there; it is held to 3e-2 of the largest gradient of the same kind (of dq | dk | dv when both tables have one row).
    zero = {"dq", "dk"} if gh * gw == 1 else set()
    zero |= ({"drel_h"} if gh == 1 else set()) | ({"drel_w"} if gw == 1 else set())
    peak = lambda names: max(ref.abs().max().item() for n, _, ref in grads if n in names)
    for name, got, ref in grads:
        if name in zero:
            scale = peak(("drel_h", "drel_w")) if name.startswith("drel") and gh * gw > 1 else peak(("dq", "dk", "dv"))
            assert ref.abs().max().item() < 1e-9 * scale and got.double().abs().max().item() < 3e-2 * scale, name
        else:
            assert relerr(got, ref) < 3e-2, name


# ------------------------------------------------------------------------------------------------ tests: inputs that make the edges matter
@pytest.mark.parametrize("shape", PADDED, ids=PADDED_IDS)
def test_mask_leak(shape):
    """Every real logit <= -25: a padded key slot that escapes the mask (logit 0) takes the whole softmax: O -> 0, lse -> >= 0."""
    nB, gh, gw, heads = shape[:4]
    tag = "leak:" + IDS[SHAPES.index(shape)]
    inputs = gen_mask_leak(shape)
    r = run_device(shape, inputs)
    O_ref, lse_ref, S = attention_ref(r["qkv"], r["rel_h"], r["rel_w"], nB, gh, gw, heads)
    assert S.max().item() <= -25.0
    assert lse_ref.max().item() <= -25.0 + torch.log(torch.tensor(float(gh * gw))).item()
    assert O_ref.min().item() > 0.5                     # v = 1 +- 0.375: a leak would be visible as O -> 0
    assert (r["O"].float() > 0.5).all() and (r["lse"] < -20).all()
    check_forward(r["att"], r["lay"], shape, r["qkv"], r["O"], r["lse"], tag)
    check_backward(r["att"], r["lay"], shape, r["qkv"], r["rel_h"], r["rel_w"], r["O"], r["lse"], r["dO"], r["dqkv"], r["drel0"],
                   r["drel"], tag)


SELECTOR = [(s, m) for s in SHAPES for m in selector_modes(s)]
SELECTOR_IDS = ["%s-%s" % (IDS[SHAPES.index(s)], m) for s, m in SELECTOR]


@pytest.mark.parametrize("shape,mode", SELECTOR, ids=SELECTOR_IDS)
def test_selector(shape, mode):
    """One key wins every query by >= 40: O[q] is v[winner] bit for bit, lse[q] the winning logit.  The permutation ("qk") and the
    displacement ("bias+-") make every key a winner, the last key tile and the last row / column of the 8x8 blocks included."""
    nB, gh, gw, heads = shape[:4]
    L = gh * gw
    qkv, rel_h, rel_w, winner = (None if t is None else t.to(DEV) for t in gen_selector(shape, mode))
    _, _, S = attention_ref(qkv, rel_h, rel_w, nB, gh, gw, heads)
    margin, win_logit = selector_margin(S, winner)
    assert margin >= 40.0
    att, lay = make_att(shape)
    O, lse = att.forward(qkv, rel_h, rel_w)
    assert torch.isfinite(O.float()).all() and torch.isfinite(lse).all()
    has = winner >= 0
    if mode != "qk" and L > 16:
        assert has.float().mean().item() > 0.3
    v = split_heads(qkv, nB, L, heads)[2]
    want = v.gather(1, winner.clamp_min(0)[..., None].expand(-1, -1, 64))
    got = split_heads(O, nB, L, heads)
    assert torch.equal(got.contiguous().view(torch.int16)[has], want.contiguous().view(torch.int16)[has])
    # the device's winning logit carries the bf16 rounding of its bias columns: compare with the matched-operand score of the winner
    S_m, _, _, _, unit = matched_scores(att, lay, shape, qkv)
    win_m = S_m.gather(2, winner.clamp_min(0)[..., None])[..., 0]
    assert ((win_m - win_logit).abs()[has] <= U8 * 128).all()
    r = worst_ratio(lse.double()[has], win_m[has], unit[has])
    report("sel:" + IDS[SHAPES.index(shape)] + ":" + mode, "lse", r)
    assert r <= LSE_C, r


WORKSPACES = ("Qp", "Kp", "KpT", "VT", "QsT", "dOT", "dQp", "delta")


def _fwd_bwd(att, shape, qkv, rel_h, rel_w, dO):
    O, lse = att.forward(qkv, rel_h, rel_w)
    drel = drel_buffers(shape, fill=False)
    dqkv = att.backward(qkv, rel_h, rel_w, O, lse, dO, drel["drel_h"], drel["drel_w"], prepared=True)
    torch.cuda.synchronize()
    return O, lse, dqkv, drel


@pytest.mark.parametrize("variant", ["nan", "stale"])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_workspace_poison(i, variant):
    """The workspaces are torch.empty: every pad element a kernel reads must be rewritten by the prep kernels of the same call.
    "nan" fills all of them with NaN between two identical runs, "stale" runs other data in between.  O, lse and dqkv must be the
    same bits; drel_h / drel_w are summed with fp32 atomics across blocks, whose order is free, so they must agree to that order's
    rounding (the accumulation envelope of check_backward, which never exceeds a few hundred E32) and be finite."""
    shape = SHAPES[i]
    qkv, rel_h, rel_w, dO = (None if t is None else t.to(DEV) for t in gen_random(shape))
    att, lay = make_att(shape)
    first = _fwd_bwd(att, shape, qkv, rel_h, rel_w, dO)
    if variant == "nan":
        for n in WORKSPACES:
            getattr(att, n).fill_(float("nan"))
    else:
        other = [None if t is None else t.to(DEV) for t in gen_random(shape, seed=1)]
        _fwd_bwd(att, shape, *other)
    second = _fwd_bwd(att, shape, qkv, rel_h, rel_w, dO)
    for name, a, b in zip(("O", "lse", "dqkv"), first, second):
        assert torch.isfinite(b.float()).all(), name
        assert same_bits(a, b), name
    if shape[4]:
        nB, gh, gw, heads = shape[:4]
        BH, L, wofs = nB * heads, gh * gw, lay["wofs"]
        dQ, qg = att.dQp.double().abs(), split_heads(qkv, nB, L, heads)[0].double().abs().reshape(BH, gh, gw, 64)
        c_tab = E32 * (4 + 9 * BH * (lay["Lp"] // 64))
        for name, db, g, eq in (("drel_h", dQ[..., 64:64 + gh].reshape(BH, gh, gw, gh), gh, "bhwk,bhwc->hkc"),
                                ("drel_w", dQ[..., 64 + wofs:64 + wofs + gw].reshape(BH, gh, gw, gw), gw, "bhwk,bhwc->wkc")):
            a, b = first[3][name], second[3][name]
            env = torch.zeros(2 * g - 1, 64, dtype=torch.float64, device=DEV).index_add(
                0, rel_index(g, DEV).reshape(-1), torch.einsum(eq, db, qg).reshape(-1, 64))
            assert torch.isfinite(b).all(), name
            assert ((a.double() - b.double()).abs() <= 2 * c_tab * env).all(), name


def test_dq_above_256_rejected():
    """1 x 192 needs Dq = 288: check_args must refuse it before any launch, in prepare, forward and backward alike"""
    import ctypes

    from aldi_amd import _lib as L
    from aldi_amd import vit_ops as V
    att = V.Attention(1, 1, 192, 1, DEV)
    assert att.Dq == 288 and not att.tiled
    qkv, rel_h, rel_w, dO = (t.to(DEV) for t in gen_random((1, 1, 192, 1, True)))
    for n in WORKSPACES:
        getattr(att, n).fill_(7.0)
    with pytest.raises(RuntimeError):
        att.forward(qkv, rel_h, rel_w)
    with pytest.raises(RuntimeError):
        att.prepare(qkv, rel_h, rel_w)
    O = torch.full((192, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    lse = torch.full((1, 192), 7.0, device=DEV)
    args = att._args(qkv, rel_h, rel_w, O, lse)
    with pytest.raises(RuntimeError):
        L.call("aldi_attn_forward", ctypes.byref(args), V.stream_ptr())
    drh, drw = torch.full((1, 64), 7.0, device=DEV), torch.full((383, 64), 7.0, device=DEV)
    with pytest.raises(RuntimeError):
        att.backward(qkv, rel_h, rel_w, O, lse, dO, drh, drw, prepared=True)
    torch.cuda.synchronize()
    for t in [getattr(att, n) for n in WORKSPACES] + [O, lse, drh, drw]:
        assert (t == 7.0).all()

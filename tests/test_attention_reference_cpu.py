"""CPU checks of what tests/test_attention_edges_gpu.py relies on: its fp64 reference equals transformers' decomposed relative
positions, its layout table reaches the dispatch arms it names, and its input generators have the properties the GPU tests assume."""
import math

import pytest
import torch

import test_attention_edges_gpu as E


def test_reference_matches_transformers():
    from transformers.models.vitdet.modeling_vitdet import add_decomposed_relative_positions
    g = torch.Generator().manual_seed(0)
    for nB, gh, gw, heads in ((2, 3, 5, 2), (1, 7, 4, 1), (1, 1, 6, 1), (1, 9, 9, 2)):
        L = gh * gw
        qkv = torch.randn(nB * L, 3 * heads * 64, generator=g, dtype=torch.float64)
        rel_h = torch.randn(2 * gh - 1, 64, generator=g, dtype=torch.float64)
        rel_w = torch.randn(2 * gw - 1, 64, generator=g, dtype=torch.float64) * 0.3
        O, lse, S = E.attention_ref(qkv, rel_h, rel_w, nB, gh, gw, heads)
        q, k, v = E.split_heads(qkv, nB, L, heads)
        s = add_decomposed_relative_positions((q * 64 ** -0.5) @ k.transpose(-2, -1), q, rel_h, rel_w, (gh, gw), (gh, gw))
        o = (s.softmax(dim=-1) @ v).view(nB, heads, gh, gw, 64).permute(0, 2, 3, 1, 4).reshape(nB * L, heads * 64)
        assert (S - s).abs().max().item() <= 1e-12 * max(1.0, s.abs().max().item())
        assert (O - o).abs().max().item() <= 1e-12
        assert (lse - torch.logsumexp(s, dim=-1)).abs().max().item() <= 1e-12 * max(1.0, s.abs().max().item())
        # no tables: plain scaled dot-product attention
        O0, _, S0 = E.attention_ref(qkv, None, None, nB, gh, gw, heads)
        assert torch.equal(S0, (q * 0.125) @ k.transpose(-2, -1))


def test_shape_table_reaches_its_arms():
    seen = set()
    for nB, gh, gw, heads, rel, tiled, Dq, _ in E.SHAPES:
        lay = E.layout(gh, gw, rel)
        assert (lay["tiled"], lay["Dq"]) == (tiled, Dq)
        assert Dq <= 256 and 1 <= nB * heads <= 4
        arm = "tiled" if tiled else ("7-wave" if lay["L"] <= 224 else "4-wave")
        seen.add((arm, Dq // 32 if not tiled else 0))
    # linear 4-wave arm (rel=False only), NKS = 4, 6, 8 of the linear kernels, both sides of the L = 224 | 225 switch, tiled Dq = 256
    assert ("4-wave", 2) in seen and {("7-wave", n) for n in (3, 4, 6, 8)} <= seen and ("tiled", 0) in seen
    by_grid = {(s[1], s[2], s[4]): s for s in E.SHAPES}
    assert not by_grid[(14, 16, True)][5] and by_grid[(15, 15, True)][5]
    assert max(s[6] for s in E.SHAPES if s[5]) == 256
    assert E.layout(1, 192, True)["Dq"] == 288
    # thin tiled grid: the tile-major k^T does not fit Dq x Lp
    lay = E.layout(2, 113, True)
    assert lay["nt2"] * 4096 > lay["Dq"] * lay["Lp"]
    assert {E.padded_slots(s) for s in E.SHAPES if (s[1], s[2]) == (15, 15)} == {31}
    assert E.padded_slots(by_grid[(16, 16, False)]) == 0 and E.padded_slots(by_grid[(8, 184, True)]) == 0


@pytest.mark.parametrize("shape", E.PADDED, ids=E.PADDED_IDS)
def test_mask_leak_generator(shape):
    nB, gh, gw, heads, rel = shape[:5]
    qkv, rel_h, rel_w, dO = E.gen_mask_leak(shape)
    assert qkv.dtype == torch.bfloat16 and (rel_h is None) == (not rel)
    if rel:
        assert torch.equal(rel_h.bfloat16().float(), rel_h) and torch.equal(rel_w.bfloat16().float(), rel_w)
    O, lse, S = E.attention_ref(qkv, rel_h, rel_w, nB, gh, gw, heads)
    assert S.max().item() <= -25.0
    assert lse.max().item() <= -25.0 + math.log(gh * gw)
    v = E.split_heads(qkv, nB, gh * gw, heads)[2].float()
    assert v.min().item() >= 0.625 and abs(v.mean().item() - 1.0) < 0.1 and O.min().item() > 0.5


@pytest.mark.parametrize("shape,mode", E.SELECTOR, ids=E.SELECTOR_IDS)
def test_selector_generator(shape, mode):
    nB, gh, gw, heads, rel = shape[:5]
    L = gh * gw
    qkv, rel_h, rel_w, winner = E.gen_selector(shape, mode)
    O, lse, S = E.attention_ref(qkv, rel_h, rel_w, nB, gh, gw, heads)
    margin, win = E.selector_margin(S, winner)
    assert margin >= 40.0
    has = winner >= 0
    if mode == "qk":
        assert has.all()
        for w in winner:                                  # a permutation: every key wins once, the last tile / row / column included
            assert torch.equal(w.sort().values, torch.arange(L))
    else:
        # the displaced key: every key that has a query at the displacement is a winner; the edges of the grid are among them
        t = torch.arange(L)
        dh = (winner[0] // gw - t // gw)[has[0]]
        dw = (winner[0] % gw - t % gw)[has[0]]
        assert dh.unique().numel() == 1 and dw.unique().numel() == 1
        keys = set(winner[0][has[0]].tolist())
        assert (L - 1 in keys) or (gw - 1 in keys) or ((gh - 1) * gw in keys) or (0 in keys)
    # the fp64 result itself selects: O is v[winner] and lse the winning logit to 1e-15 relative
    v = E.split_heads(qkv, nB, L, heads)[2].double()
    want = v.gather(1, winner.clamp_min(0)[..., None].expand(-1, -1, 64))
    got = E.split_heads(O, nB, L, heads)
    assert ((got - want).abs()[has] < 1e-12).all()
    assert ((lse - win).abs()[has] < 1e-12).all()

"""Gradient clipping for the flat SGD state, host side: the D2 parameters as segments of the flat layout (pinned to pack / unpack),
the chunk-table builder, and SOLVER.CLIP_GRADIENTS -> EngineSGD."""
import pytest
import torch


# ---- ParamLayout.param_segments
@pytest.mark.parametrize("K", [8, 80])
@pytest.mark.parametrize("da", [False, True])
def test_param_segments_are_the_index_sets_unpack_reads(K, da):
    from aldi_amd.arch import ParamLayout, d2_convs, disc_convs
    lay = ParamLayout(K, da, da)
    segs = lay.param_segments()
    # disjoint, ascending, inside [0, n_train)
    pos = 0
    for key, off, numel in segs:
        assert off >= pos and numel > 0, (key, off, pos)
        pos = off + numel
    assert pos <= lay.n_train
    # one entry per trainable detectron2 parameter: res3-res5 weights, FPN / RPN / box head weights and biases, the discriminators
    convs = dict(d2_convs(K))
    convs.update(disc_convs(da, da))
    want = []
    for name, c in convs.items():
        if c.trainable:
            want.append(name + ".weight")
            if c.bias:
                want.append(name + ".bias")
    assert sorted(k for k, _, _ in segs) == sorted(want) and len(set(want)) == len(want)
    assert not any("stem" in k or ".res2." in k or ".norm." in k for k, _, _ in segs)
    assert ("img_align.model.0.weight" in want) == bool(da) and ("ins_align.model.1.bias" in want) == bool(da)
    # element i holds i: every key's tensor must hold exactly its segment's indices (fc1 permutes inside its own)
    sd = lay.unpack(torch.arange(lay.n_total, dtype=torch.int32))
    by_key = {k: (off, numel) for k, off, numel in segs}
    for key, t in sd.items():
        if key in by_key:
            off, numel = by_key[key]
            assert t.numel() == numel, key
            assert torch.equal(torch.sort(t.reshape(-1)).values, torch.arange(off, off + numel, dtype=torch.int32)), key
        else:
            assert int(t.min()) >= lay.n_train, key                       # frozen weights and FrozenBN buffers: no parameter
    fc1 = sd["roi_heads.box_head.fc1.weight"].reshape(-1)
    assert not torch.equal(fc1, torch.sort(fc1).values)                    # (it IS permuted)
    # what is left of [0, n_train) is the zero padding: a round trip through the state dict keeps exactly the segments' elements
    kept = lay.pack(lay.unpack(torch.ones(lay.n_total)))[: lay.n_train] != 0
    mine = torch.zeros(lay.n_train, dtype=torch.bool)
    for _, off, numel in segs:
        mine[off: off + numel] = True
    assert torch.equal(kept, mine)
    assert int((~mine).sum()) > 0


def test_packed_heads_split_into_their_sources():
    from aldi_amd.arch import ParamLayout
    K = 8
    lay = ParamLayout(K)
    s = {k: (off, numel) for k, off, numel in lay.param_segments()}
    rp, bp = lay.t["rpn_head_out"], lay.t["box_pred"]
    assert s["proposal_generator.rpn_head.objectness_logits.weight"] == (rp.w_off, 3 * 256)
    assert s["proposal_generator.rpn_head.anchor_deltas.weight"] == (rp.w_off + 3 * 256, 12 * 256)
    assert s["proposal_generator.rpn_head.objectness_logits.bias"] == (rp.b_off, 3)
    assert s["proposal_generator.rpn_head.anchor_deltas.bias"] == (rp.b_off + 3, 12)
    assert s["roi_heads.box_predictor.cls_score.bias"] == (bp.b_off, K + 1)
    assert s["roi_heads.box_predictor.bbox_pred.bias"] == (bp.b_off + K + 1, 4 * K)
    assert s["roi_heads.box_predictor.bbox_pred.weight"] == (bp.w_off + (K + 1) * 1024, 4 * K * 1024)


# ---- the chunk table
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


def test_chunk_table_tiles_segments_and_padding():
    from aldi_amd import ops
    CH = ops.CLIP_CHUNK
    assert CH >= 256 and CH % 4 == 0
    segs, n = _segments(CH)
    assert sorted({s % 4 for s, _ in segs}) == [1, 2, 3]
    chunks, seg_chunks = ops.clip_chunk_table(segs, n)
    owner = torch.full((n,), -2, dtype=torch.int64)
    prev_end = 0
    for start, ln, seg in chunks:
        assert 0 < ln <= CH and start == prev_end                          # ascending, gapless: [0, n) exactly once
        assert (owner[start: start + ln] == -2).all()
        owner[start: start + ln] = seg
        prev_end = start + ln
    assert prev_end == n
    want = torch.full((n,), -1, dtype=torch.int64)
    for i, (s, ln) in enumerate(segs):
        want[s: s + ln] = i
    assert torch.equal(owner, want)                                          # segments by their own index, the complement as padding
    for i, (s, ln) in enumerate(segs):
        first, cnt = seg_chunks[i]
        mine = chunks[first: first + cnt]
        assert cnt == (ln + CH - 1) // CH and all(c[2] == i for c in mine)
        assert mine[0][0] == s and sum(c[1] for c in mine) == ln
        assert [c for c in chunks if c[2] == i] == mine
        assert all(c[1] == CH for c in mine[:-1])                           # only a segment's last chunk is short
    assert seg_chunks[-1][1] == 4 and seg_chunks[6][1] == 1 and seg_chunks[7][1] == 2
    # no segments: all padding;  one segment = everything: no padding
    chunks, seg_chunks = ops.clip_chunk_table([], 2 * CH + 1)
    assert [c[1:] for c in chunks] == [(CH, -1), (CH, -1), (1, -1)] and seg_chunks == []
    chunks, seg_chunks = ops.clip_chunk_table([(0, CH)], CH)
    assert chunks == [(0, CH, 0)] and seg_chunks == [(0, 1)]
    for bad in ([(4, 4), (6, 4)], [(8, 4), (0, 4)], [(0, 0)], [(0, 9)]):
        with pytest.raises(ValueError):
            ops.clip_chunk_table(bad, 8)


# ---- SOLVER.CLIP_GRADIENTS -> EngineSGD
class _Weights:
    def __init__(self):
        self.calls = []
        self.first_step = True

    def sgd_step(self, lr, momentum, wd, **kw):
        self.calls.append(kw)


class _Model:
    def __init__(self):
        self.weights = _Weights()


def _cfg(*opts):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_list(["SOLVER.BASE_LR", 0.1] + list(opts))
    return cfg


@pytest.mark.parametrize("which", ["DefaultTrainer", "ALDITrainer"])
def test_build_optimizer_reads_clip_gradients(which):
    from aldi_amd import trainer as T
    from aldi_amd.ops import ClipSpec
    build = getattr(T, which).build_optimizer
    cfg = _cfg()
    assert cfg.SOLVER.CLIP_GRADIENTS.ENABLED is False
    m = _Model()
    opt = build(cfg, m)
    assert type(opt) is T.EngineSGD and opt.clip is None and "clip" not in opt.param_groups[0]
    opt.step()
    assert m.weights.calls == [{}]                                           # today's call, no clip argument at all
    del cfg.SOLVER["CLIP_GRADIENTS"]                                         # no node: the same
    assert build(cfg, _Model()).clip is None
    inf = float("inf")
    for ctype, ntype, want in (("value", 2.0, ClipSpec("value", 0.5, 2.0)), ("norm", 2.0, ClipSpec("norm", 0.5, 2.0)), ("norm", inf, ClipSpec("norm", 0.5, inf)),
                               ("norm", "inf", ClipSpec("norm", 0.5, inf)), ("full_model", 2.0, ClipSpec("full_model", 0.5, 2.0)),
                               ("full_model", inf, ClipSpec("full_model", 0.5, inf)), ("value", inf, ClipSpec("value", 0.5, inf))):
        cfg = _cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", ctype, "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.5)
        cfg.SOLVER.CLIP_GRADIENTS.NORM_TYPE = ntype
        m = _Model()
        opt = build(cfg, m)
        assert type(opt) is T.EngineSGD and opt.clip == want and opt.param_groups[0]["clip"] == want
        assert {k: opt.param_groups[0][k] for k in ("lr", "momentum", "weight_decay")} == {"lr": 0.1, "momentum": cfg.SOLVER.MOMENTUM, "weight_decay": cfg.SOLVER.WEIGHT_DECAY}
        opt.step()
        assert m.weights.calls == [{"clip": want}]
    for key, val in (("CLIP_TYPE", "foo"), ("NORM_TYPE", 3.0), ("CLIP_VALUE", 0.0), ("CLIP_VALUE", -1.0), ("NORM_TYPE", "two")):
        cfg = _cfg("SOLVER.CLIP_GRADIENTS.ENABLED", True)
        cfg.SOLVER.CLIP_GRADIENTS[key] = val
        with pytest.raises(ValueError) as e:
            build(cfg, _Model())
        assert "SOLVER.CLIP_GRADIENTS." + key in str(e.value) and repr(val) in str(e.value)
        cfg.SOLVER.CLIP_GRADIENTS.ENABLED = False                            # a disabled node is not validated (detectron2 does not either)
        assert build(cfg, _Model()).clip is None


def test_clip_spec_is_not_checkpoint_state():
    from aldi_amd import trainer as T
    from aldi_amd.ops import ClipSpec

    class W(_Weights):
        _mom = None
    m = _Model()
    m.weights = W()
    opt = T.EngineSGD(m, 0.1, 0.9, 1e-4, clip=ClipSpec("norm", 1.0, 2.0))
    sd = opt.state_dict()
    assert sd["param_groups"] == [{"lr": 0.1, "momentum": 0.9, "weight_decay": 1e-4}]
    plain = T.EngineSGD(m, 0.1, 0.9, 1e-4)
    assert plain.state_dict()["param_groups"] == sd["param_groups"]
    plain.load_state_dict(sd)
    assert plain.clip is None


def test_sgd_inside_the_step_is_off_while_clipping(monkeypatch):
    """ALDI_SGD_IN_STEP=1 must not bypass the clip: _defers_sgd is False for every clip type"""
    from aldi_amd import trainer as T
    from aldi_amd.ops import ClipSpec
    monkeypatch.setenv("ALDI_SGD_IN_STEP", "1")

    class Tr(T._ALDITrainer):
        def __init__(self, opt):
            self.optimizer, self.model = opt, opt.model

        def _defers_zero_grad(self):
            return True
    m = _Model()
    m.weights.first_step = False
    assert Tr(T.EngineSGD(m, 0.1))._defers_sgd() is True
    for ctype in ("value", "norm", "full_model"):
        assert Tr(T.EngineSGD(m, 0.1, clip=ClipSpec(ctype, 1.0, 2.0)))._defers_sgd() is False

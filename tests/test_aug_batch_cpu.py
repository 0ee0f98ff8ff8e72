"""Host half of the batched strong augmentation (aldi_amd/aug.py draw_strong_params, csrc/host_rng.cpp aldi_np_mt_advance):
the parameters and the generator streams equal the oracle's restatement of the reference chain, which really calls
np.random.rand for the erase fills; the recorded snapshots replay those fills bit for bit.  No GPU needed."""
import random

import numpy as np
import pytest

from oracle import aug_ops as ao

SEEDS = list(range(24))


def _chain(erasing, mic):
    from aldi_amd import aug
    augs = aug.build_strong_augmentation(include_erasing=erasing)
    if mic is not None:
        augs.append(aug.RandomApply(aug.MICTransform(*mic), prob=1.0))
    return augs


def _same_op(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "mic":
        return a[1].shape == b[1].shape and np.array_equal(a[1], b[1])
    return a[1] == b[1]


@pytest.mark.parametrize("erasing", [True, False])
@pytest.mark.parametrize("mic", [None, (0.5, 32), (0.3, 16)])
def test_params_fills_and_streams_equal_the_oracle(erasing, mic):
    from aldi_amd import aug
    augs = _chain(erasing, mic)
    for seed in SEEDS:
        H, W = 120 + 13 * seed, 200 + 7 * seed
        np.random.seed(seed); random.seed(seed)
        ref = ao.draw_strong_params(H, W, include_erasing=erasing, mic=mic)
        ref_np, ref_py = np.random.get_state(), random.getstate()
        np.random.seed(seed); random.seed(seed)
        p = aug.draw_strong_params(augs, H, W)
        got = p.ops()
        assert len(got) == len(ref) and all(_same_op(g, r) for g, r in zip(got, ref)), (seed, [o[0] for o in ref], [o[0] for o in got])
        fills = [o[2] for o in ref if o[0] == "erase"]
        assert len(fills) == len(p.erases)
        for (rect, snaps, snap_pos), fill in zip(p.erases, fills):
            rs = np.random.RandomState()
            rs.set_state(("MT19937", snaps[0], int(snap_pos[0])))
            assert np.array_equal(rs.rand(rect[2], rect[3], 3), fill), (seed, rect)
            assert len(snaps) == (2 * fill.size + aug.FILL_SEG_WORDS - 1) // aug.FILL_SEG_WORDS
        st = np.random.get_state()
        assert np.array_equal(st[1], ref_np[1]) and st[2] == ref_np[2] and random.getstate() == ref_py, seed


def test_private_generators_equal_the_seeded_global_streams():
    from aldi_amd import aug
    augs = _chain(True, (0.5, 32))
    for seed in SEEDS:
        np.random.seed(seed); random.seed(seed)
        a = aug.draw_strong_params(augs, 512, 640)
        rs, pr = np.random.RandomState(seed), random.Random(seed)
        glob = np.random.get_state()
        b = aug.draw_strong_params(augs, 512, 640, np_rng=rs, py_rng=pr)
        assert all(_same_op(x, y) for x, y in zip(a.ops(), b.ops())) and len(a.ops()) == len(b.ops())
        for (ra, sa, pa), (rb, sb, pb) in zip(a.erases, b.erases):
            assert ra == rb and np.array_equal(sa, sb) and np.array_equal(pa, pb)
        assert np.array_equal(rs.get_state()[1], np.random.get_state()[1]) and rs.get_state()[2] == np.random.get_state()[2]
        assert pr.getstate() == random.getstate()
        assert np.array_equal(glob[1], np.random.get_state()[1])       # the private draw left the global stream alone


def test_generator_is_rejected():
    from aldi_amd import aug
    with pytest.raises(TypeError, match="Generator"):
        aug.draw_strong_params(_chain(True, None), 64, 64, np_rng=np.random.default_rng(0))


@pytest.mark.parametrize("skip", [0, 1, 3, 623, 624, 1247])
@pytest.mark.parametrize("n_doubles", [0, 1, 311, 312, 313, 5000, 20011])
def test_snapshot_advance_matches_rand(skip, n_doubles):
    """odd start positions, fills across refill boundaries, n = 0; every snapshot resumes the stream where rand would be"""
    from aldi_amd import aug
    rs = np.random.RandomState(77)
    rs.rand(skip // 2)
    if skip % 2:
        rs.randint(0, 2 ** 32, dtype=np.uint32)      # one 32-bit output: odd position
    ref = np.random.RandomState()
    ref.set_state(rs.get_state())
    seg = 1000
    snaps, pos = aug.np_mt_advance(rs, 2 * n_doubles, seg)
    expect = ref.rand(n_doubles)
    assert len(snaps) == (2 * n_doubles + seg - 1) // seg
    for k in range(len(snaps)):
        r = np.random.RandomState()
        r.set_state(("MT19937", snaps[k], int(pos[k])))
        m = min(seg // 2, n_doubles - k * seg // 2)
        assert np.array_equal(r.rand(m), expect[k * seg // 2: k * seg // 2 + m]), k
    a, b = rs.get_state(), ref.get_state()
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert rs.rand() == ref.rand()


def test_chain_recognition():
    from aldi_amd import aug
    assert aug.recognise_chain(_chain(True, (0.5, 32))) is not None
    assert aug.recognise_chain(_chain(False, None)) is not None
    assert aug.recognise_chain([aug.RandomApply(aug.RandomBlurTransform((0.1, 3.0)))]) is None      # radius 12 > halo
    assert aug.recognise_chain([aug.RandomApply(aug.RandomEraseTransform(value=0.5))]) is None
    assert aug.recognise_chain(list(reversed(_chain(True, None)))) is None                           # order matters


def test_default_config_keeps_the_device_strong_stage_off():
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    assert cfg.AUG.DEVICE_STRONG is False

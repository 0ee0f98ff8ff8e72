"""Device views with a source window (aldi_amd/aug.py views -> csrc/geom.hip): byte-identical to Pillow's BILINEAR
resize of `raw[y0:y0+h, x0:x0+w]` (tests/golden/pil_window.npz: Pillow's own bytes) in both kernel arms, every layout, every flip and
with and without the R <-> B exchange; nothing outside the window is read, nothing outside `dst` is written.  Every comparison is
bit-exact."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_pil_window_golden import CASES, make_raw  # noqa: E402

TWO_PASS_ALWAYS = 1                                                    # case 2: its row window exceeds the LDS budget
_cache = {}


def golden():
    """[(raw_h, raw_w, y0, x0, h, w, new_h, new_w, raw HWC, Pillow's output HWC)], loaded once and left unchanged"""
    if "g" not in _cache:
        g = np.load(os.path.join(ROOT, "tests", "golden", "pil_window.npz"))
        _cache["g"] = [tuple(c[:8]) + (make_raw(c[0], c[1], c[8]), g[f"out_{i}"]) for i, c in enumerate(g["cases"].tolist())]
        assert len(_cache["g"]) == len(CASES) == 10
    return _cache["g"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def expected(out, hflip, vflip, swap, chw):
    e = out
    if hflip:
        e = e[:, ::-1]
    if vflip:
        e = e[::-1]
    if swap:
        e = e[:, :, ::-1]
    return torch.from_numpy(np.array(e.transpose(2, 0, 1) if chw else e, order="C", copy=True))   # (a copy: no negative strides left)


@pytest.fixture
def tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield L
    L.reset_tuning()


def _spy(monkeypatch):
    """records (ntiles, nh_blocks, nv_blocks) of every aldi_geom_batch_resize call"""
    from aldi_amd import _lib as L
    calls, real = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(a[3:6]) if name == "aldi_geom_batch_resize" else None, real(name, *a))[1])
    return calls


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("case", range(10), ids=lambda i: "case%d" % (i + 1))
def test_every_case_layout_flip_and_channel_order_equals_pillow(case, fused, tuning, monkeypatch):
    from aldi_amd import aug
    tuning.set_tuning("resize_fused", fused)
    calls = _spy(monkeypatch)
    rh, rw, y0, x0, h, w, nh, nw, raw, out = golden()[case]
    src = {False: dev(raw), True: dev(raw.transpose(2, 0, 1))}
    for chw_out in (True, False):
        imgs, params, expect = [], [], []
        for chw_in in (False, True):
            for hflip in (False, True):
                for vflip in (False, True):
                    for swap in (False, True):
                        imgs.append(src[chw_in])
                        params.append(aug.ViewParams(rh, rw, y0, x0, h, w, nh, nw, hflip, vflip, swap))
                        expect.append(expected(out, hflip, vflip, swap, chw_out))
        got = aug.views(imgs, params, chw_out=chw_out)
        for k, (g_, e) in enumerate(zip(got, expect)):
            assert g_.dtype == torch.uint8 and tuple(g_.shape) == tuple(e.shape)
            assert torch.equal(g_.cpu(), e), (case, fused, chw_out, k, params[k])
    takes_fused = bool(fused) and case != TWO_PASS_ALWAYS
    for ntiles, nh_, nv_ in calls:
        assert (ntiles > 0, nh_ > 0, nv_ > 0) == (takes_fused, not takes_fused, not takes_fused), (case, fused, calls)
    assert len(calls) == 2


@pytest.mark.parametrize("fused", [1, 0])
def test_whole_image_window_equals_launch_weak_views(fused, tuning):
    from aldi_amd import aug
    tuning.set_tuning("resize_fused", fused)
    rh, rw, y0, x0, h, w, nh, nw, raw, out = golden()[2]
    assert (y0, x0, h, w) == (0, 0, rh, rw)
    for chw in (False, True):
        img = dev(raw.transpose(2, 0, 1) if chw else raw)
        for flip in (False, True):
            wp = aug.WeakParams(rh, rw, nh, nw, flip)
            a = aug.weak_views([img], [wp], chw_out=chw)[0]
            b = aug.views([img], [aug.ViewParams.whole(wp)], chw_out=chw)[0]
            assert torch.equal(a, b) and torch.equal(a.cpu(), expected(out, flip, False, False, chw))


@pytest.mark.parametrize("fused", [1, 0])
def test_nothing_outside_the_window_is_read(fused, tuning):
    """the same window contents inside two raws with different surroundings (random bytes; 0x00 and 0xFF would show a tap with any
    weight) give identical outputs"""
    from aldi_amd import aug
    tuning.set_tuning("resize_fused", fused)
    for case in (0, 1, 3, 4, 6, 7, 8, 9):
        rh, rw, y0, x0, h, w, nh, nw, raw, out = golden()[case]
        for chw in (False, True):
            got = []
            for fill in (None, 0x00, 0xFF):
                other = raw.copy() if fill is None else np.full_like(raw, fill)
                other[y0:y0 + h, x0:x0 + w] = raw[y0:y0 + h, x0:x0 + w]
                got.append(aug.views([dev(other.transpose(2, 0, 1) if chw else other)], [aug.ViewParams(rh, rw, y0, x0, h, w, nh, nw)], chw_out=chw)[0])
            assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]), (case, chw)
            assert torch.equal(got[0].cpu(), expected(out, False, False, False, chw)), (case, chw)


@pytest.mark.parametrize("fused", [1, 0])
def test_guard_bands_around_dst_and_raw_at_both_ends_of_its_allocation(fused, tuning):
    from aldi_amd import aug
    tuning.set_tuning("resize_fused", fused)
    PAD = 4096
    for case in (0, 1, 4, 6, 7):                                       # (5 and 7: the window ends at the raw image's last byte)
        rh, rw, y0, x0, h, w, nh, nw, raw, out = golden()[case]
        nsrc, ndst = rh * rw * 3, nh * nw * 3
        for chw in (False, True):
            flat = torch.from_numpy(np.ascontiguousarray(raw.transpose(2, 0, 1) if chw else raw).reshape(-1))
            for at_end in (False, True):
                for fill in (0x00, 0xFF):                              # a read past either end with a non-zero weight would show
                    sbuf = torch.full((nsrc + PAD,), fill, dtype=torch.uint8, device=DEV)
                    view = sbuf[PAD:] if at_end else sbuf[:nsrc]
                    view.copy_(flat)
                    src = view.view((3, rh, rw) if chw else (rh, rw, 3))
                    dbuf = torch.full((ndst + 2 * PAD,), 0xA5, dtype=torch.uint8, device=DEV)
                    dst = dbuf[PAD: PAD + ndst].view((3, nh, nw) if chw else (nh, nw, 3))
                    p = aug.ViewParams(rh, rw, y0, x0, h, w, nh, nw, hflip=at_end, vflip=not at_end, swap_rb=fill == 0xFF)
                    got = aug.views([src], [p], chw_out=chw, outs=[dst])[0]
                    assert got.data_ptr() == dst.data_ptr()
                    assert torch.equal(dst.cpu(), expected(out, p.hflip, p.vflip, p.swap_rb, chw)), (case, chw, at_end, fill)
                    assert bool((dbuf[:PAD] == 0xA5).all()) and bool((dbuf[PAD + ndst:] == 0xA5).all()), (case, chw, at_end)


@pytest.mark.parametrize("fused", [1, 0])
def test_one_ragged_batch_equals_the_five_single_calls(fused, tuning, monkeypatch):
    """windowed and whole images, fused and two-pass arms, both source layouts, every store permutation, in one call"""
    from aldi_amd import aug
    tuning.set_tuning("resize_fused", fused)
    pick = [0, 1, 2, 3, 9]
    flags = [(False, True, True), (True, False, False), (True, True, False), (False, False, True), (True, True, True)]
    imgs, params = [], []
    for i, (c, (hf, vf, sw)) in enumerate(zip(pick, flags)):
        rh, rw, y0, x0, h, w, nh, nw, raw, _ = golden()[c]
        imgs.append(dev(raw.transpose(2, 0, 1) if i % 2 else raw))
        params.append(aug.ViewParams(rh, rw, y0, x0, h, w, nh, nw, hf, vf, sw))
    calls = _spy(monkeypatch)
    batch = aug.views(imgs, params)
    assert len(calls) == 1 and (calls[0][0] > 0) == bool(fused) and calls[0][1] > 0               # (one call; case 2 is two-pass in it)
    single = [aug.views([v], [p])[0] for v, p in zip(imgs, params)]
    for i, (b, s, c) in enumerate(zip(batch, single, pick)):
        p = params[i]
        assert torch.equal(b, s) and torch.equal(b.cpu(), expected(golden()[c][9], p.hflip, p.vflip, p.swap_rb, True)), i


def test_a_window_outside_the_image_raises_and_launches_nothing(monkeypatch):
    from aldi_amd import aug
    calls = _spy(monkeypatch)
    img = torch.zeros((8, 9, 3), dtype=torch.uint8, device=DEV)
    for bad in (aug.ViewParams(8, 9, 5, 0, 4, 9, 4, 4), aug.ViewParams(8, 9, 0, 6, 4, 4, 4, 4), aug.ViewParams(8, 9, -1, 0, 4, 4, 4, 4),
                aug.ViewParams(8, 9, 0, 0, 0, 4, 4, 4)):
        with pytest.raises(ValueError) as e:
            aug.views([img, img], [aug.ViewParams(8, 9, 0, 0, 8, 9, 4, 4), bad])
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match="`outs`"):
        aug.views([img], [aug.ViewParams(8, 9, 1, 1, 4, 4, 4, 4)], outs=[torch.zeros((3, 4, 5), dtype=torch.uint8, device=DEV)])
    assert calls == []

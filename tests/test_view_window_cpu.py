"""Host half of the windowed device view (aldi_amd/aug.py launch_views -> csrc/geom.hip): Pillow's bytes for a
window of a raw image (tests/golden/pil_window.npz) against the scalar restatement (tests/pil_resize_ref.py) and live Pillow; the
descriptor's layout and its tail as the kernels read it (aldi_geom_window is the kernels' own function, compiled for the host); the
argument errors of `launch_views` that are raised before any device call."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pil_resize_ref as R  # noqa: E402
from make_pil_window_golden import CASES, make_raw, seed_of  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_window.npz")


def _cases():
    g = np.load(GOLDEN)
    return g, g["cases"].tolist()


def test_fixture_holds_the_ten_cases_and_is_no_larger_than_the_weak_fixture():
    g, cases = _cases()
    assert [((c[0], c[1]), (c[2], c[3]), (c[4], c[5]), (c[6], c[7])) for c in cases] == CASES and len(CASES) == 10
    assert [c[8] for c in cases] == [seed_of(i) for i in range(10)]
    assert str(g["pillow_version"])
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "pil_bilinear.npz"))


def test_fixture_equals_the_restatement_applied_to_the_window():
    g, cases = _cases()
    for i, (rh, rw, y0, x0, h, w, nh, nw, seed) in enumerate(cases):
        raw = make_raw(rh, rw, seed)
        assert y0 >= 0 and x0 >= 0 and y0 + h <= rh and x0 + w <= rw
        out = g[f"out_{i}"]
        assert out.shape == (nh, nw, 3) and out.dtype == np.uint8
        assert np.array_equal(R.resize(np.ascontiguousarray(raw[y0:y0 + h, x0:x0 + w]), nh, nw), out), (i, cases[i])
    assert np.array_equal(g["out_3"], make_raw(70, 90, seed_of(3))[20:70, 20:90])                # the pure crop is a slice


def test_fixture_equals_live_pillow_where_installed():
    try:
        from PIL import Image
    except ImportError:
        print("Pillow is not installed: the fixture holds Pillow's recorded bytes, the test above holds the restatement to them")
        return
    g, cases = _cases()
    for i, (rh, rw, y0, x0, h, w, nh, nw, seed) in enumerate(cases):
        win = make_raw(rh, rw, seed)[y0:y0 + h, x0:x0 + w]
        assert np.array_equal(np.asarray(Image.fromarray(win).resize((nw, nh), Image.BILINEAR)), g[f"out_{i}"]), i


def test_geom_desc_mirrors_the_c_struct():
    from aldi_amd import _lib as L
    from aldi_amd import aug
    src = open(L.HEADER_PATH).read()
    body = re.search(r"typedef struct aldi_geom_desc \{(.*?)\} aldi_geom_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [part.strip().split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in aug._GeomDesc._fields_]
    assert names[-4:] == ["src_h", "src_w", "y0", "x0"] and names[:8] == ["src", "dst", "tmp", "h", "w", "new_h", "new_w", "flags"]
    # three pointers and eighteen ints, no padding: the size csrc/geom.hip's static_assert pins on the C side
    assert ctypes.sizeof(aug._GeomDesc) == 3 * ctypes.sizeof(ctypes.c_void_p) + 18 * ctypes.sizeof(ctypes.c_int) == 96
    assert aug._GeomDesc.src_h.offset == 80 and aug._GeomDesc.x0.offset == 92
    assert "static_assert(sizeof(aldi_geom_desc) == 3 * sizeof(void*) + 18 * sizeof(int)" in open(os.path.join(ROOT, "aldi_amd", "csrc", "geom.hip")).read()
    flags = dict(re.findall(r"ALDI_GEOM_(\w+) = (\d+)", src))
    assert (int(flags["VFLIP"]), int(flags["SWAP_RB"])) == (16, 32) == (aug._GEOM_VFLIP, aug._GEOM_SWAP_RB)
    assert [int(flags[k]) for k in ("CHW_IN", "CHW_OUT", "HFLIP", "FUSED")] == [1, 2, 4, 8]


def _window(**kw):
    """(base, plane, stride, inside) as the kernels compute them for a descriptor with these fields"""
    from aldi_amd import _lib as L
    from aldi_amd import aug
    d = aug._GeomDesc()
    for k, v in kw.items():
        setattr(d, k, v)
    base, plane, stride, inside = ctypes.c_long(-1), ctypes.c_long(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    L.call("aldi_geom_window", ctypes.byref(d), ctypes.byref(base), ctypes.byref(plane), ctypes.byref(stride), ctypes.byref(inside))
    return base.value, plane.value, stride.value, inside.value


def test_zero_tail_is_the_whole_image_and_a_window_outside_is_refused():
    assert _window(h=37, w=53) == (0, 37 * 53, 53, 1)                                             # filled as before the tail existed
    assert _window(h=37, w=53, src_h=37, src_w=53) == (0, 37 * 53, 53, 1)                         # the same, spelled out
    assert _window(h=23, w=37, src_h=40, src_w=50, y0=9, x0=7) == (9 * 50 + 7, 40 * 50, 50, 1)
    assert _window(h=33, w=53, src_h=60, src_w=80, y0=27, x0=27)[3] == 1                          # ends at the last row and column
    assert _window(h=1, w=1, src_h=9, src_w=9, y0=8, x0=8) == (80, 81, 9, 1)
    for bad in (dict(h=33, w=53, src_h=60, src_w=80, y0=28, x0=27), dict(h=33, w=53, src_h=60, src_w=80, y0=27, x0=28),
                dict(h=4, w=4, src_h=9, src_w=9, y0=-1, x0=0), dict(h=4, w=4, src_h=9, src_w=9, y0=0, x0=-1),
                dict(h=4, w=4, src_h=0, src_w=0, y0=1, x0=0),                                     # an origin without a raw size
                dict(h=4, w=2 ** 31 - 1, src_h=9, src_w=9, y0=0, x0=2 ** 31 - 1),                  # x0 + w past int: no wrap-around
                dict(h=0, w=4), dict(h=4, w=0, src_h=9, src_w=9)):
        assert _window(**bad)[3] == 0, bad
    from aldi_amd import _lib as L
    assert L.lib.aldi_geom_window(None, None, None, None, None) == -2


def test_whole_turns_weak_parameters_into_a_window_that_covers_the_image():
    from aldi_amd import aug
    p = aug.ViewParams.whole(aug.WeakParams(64, 128, 25, 50, True))
    assert (p.raw_h, p.raw_w, p.y0, p.x0, p.h, p.w, p.new_h, p.new_w, p.hflip, p.vflip, p.swap_rb) == (64, 128, 0, 0, 64, 128, 25, 50, True, False, False)


def test_launch_views_argument_errors_come_before_any_device_call():
    """host tensors throughout: every one of these is raised while the arguments are read"""
    from aldi_amd import aug
    img = torch.zeros((8, 9, 3), dtype=torch.uint8)
    V = aug.ViewParams
    assert aug.launch_views([], []) == [] and aug.views([], []) == []
    with pytest.raises(ValueError, match="one ViewParams per image"):
        aug.launch_views([img], [])
    with pytest.raises(ValueError, match="expected a ViewParams, got WeakParams"):
        aug.launch_views([img], [aug.WeakParams(8, 9, 4, 4)])
    for bad in (V(8, 9, 5, 0, 4, 9, 4, 4), V(8, 9, 0, 1, 8, 9, 4, 4), V(8, 9, -1, 0, 4, 4, 4, 4), V(8, 9, 0, -2, 4, 4, 4, 4)):
        with pytest.raises(ValueError, match="window is not inside the 8x9 image") as e:
            aug.launch_views([img], [bad])
        assert repr(bad) in str(e.value)                                                          # the ViewParams is printed
    for bad in (V(8, 9, 0, 0, 0, 4, 4, 4), V(8, 9, 0, 0, 4, 0, 4, 4), V(8, 9, 0, 0, 4, 4, 0, 4), V(8, 9, 0, 0, 4, 4, 4, 0)):
        with pytest.raises(ValueError, match="empty window") as e:
            aug.launch_views([img], [bad])
        assert repr(bad) in str(e.value)
    with pytest.raises(ValueError, match=r"parameters drawn for 9x8.*raw size 9x8"):              # the layout is read against the RAW size
        aug.launch_views([img], [V(9, 8, 0, 0, 4, 4, 4, 4)])
    with pytest.raises(ValueError, match="parameters drawn for"):
        aug.launch_views([img], [V(8, 9, 0, 0, 4, 4, 4, 4)], chw_in=True)
    with pytest.raises(ValueError, match="uint8 images of three dimensions"):
        aug.launch_views([img.float()], [V(8, 9, 0, 0, 4, 4, 4, 4)])
    with pytest.raises(ValueError, match="contiguous CUDA"):
        aug.launch_views([img], [V(8, 9, 2, 3, 4, 4, 4, 4)])

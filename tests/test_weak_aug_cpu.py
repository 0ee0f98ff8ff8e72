"""Host half of the device weak view (aldi_amd/aug.py, AUG.DEVICE_WEAK): the numpy restatement of Pillow's bilinear resize
(tests/pil_resize_ref.py) against Pillow's own bytes (tests/golden/pil_bilinear.npz, and live Pillow where installed), the
product's coefficient tables against the restatement, and the detectron2 pieces -- output shape, draw order, box transform,
config -- against directed cases.  Everything is integer or float64 arithmetic compared for equality."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import pil_resize_ref as R  # noqa: E402
from make_pil_golden import SHAPES, make_input  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_bilinear.npz")


def test_restatement_equals_pillows_bytes_in_the_fixture():
    g = np.load(GOLDEN)
    cases = g["cases"]
    assert len(cases) == 2 * len(SHAPES)
    assert {((h, w), (nh, nw)) for h, w, nh, nw, _, _ in cases.tolist()} == set(SHAPES)
    for i, (h, w, nh, nw, seed, binary) in enumerate(cases.tolist()):
        img = make_input(h, w, seed, bool(binary))
        if binary:
            assert set(np.unique(img)) <= {0, 255}
        assert np.array_equal(R.resize(img, nh, nw), g[f"out_{i}"]), (i, h, w, nh, nw)


def test_restatement_equals_live_pillow_where_installed():
    try:
        from PIL import Image
    except ImportError:
        print("Pillow is not installed: the fixture test above holds the restatement to Pillow's recorded bytes")
        return
    rs = np.random.RandomState(0)
    shapes = [(tuple(rs.randint(1, 41, 2)), tuple(rs.randint(1, 61, 2))) for _ in range(40)] + [((480, 640), (800, 1067))]
    for k, ((h, w), (nh, nw)) in enumerate(shapes):
        img = make_input(int(h), int(w), 1000 + k, k % 3 == 0)
        ref = np.asarray(Image.fromarray(img).resize((int(nw), int(nh)), Image.BILINEAR))
        assert np.array_equal(R.resize(img, int(nh), int(nw)), ref), (h, w, nh, nw)


@pytest.mark.parametrize("insz,outsz", [(37, 80), (53, 115), (128, 50), (70, 35), (33, 99), (201, 13), (100, 7), (3, 64), (5, 64), (1, 4),
                                        (9, 36), (9, 27), (1, 3), (480, 200), (53, 1), (1, 1), (2048, 1600), (640, 1067), (500, 1333)])
def test_resize_tables_equal_the_restatements_coefficients(insz, outsz):
    from aldi_amd import aug
    ksize, bounds, kk = R.coefficients(insz, outsz)
    k, b = aug.resize_tables(insz, outsz)
    assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (outsz, ksize) and b.shape == (outsz, 2)
    assert np.array_equal(k, np.array(kk)) and np.array_equal(b, np.array(bounds))
    assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= insz).all() and (b[:, 1] <= ksize).all()        # every tap inside the image
    assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()                     # the fused tile's row window relies on it
    assert aug.resize_tables(insz, outsz)[0] is k                                                         # cached


def test_get_output_shape_directed_cases():
    from aldi_amd.aug import ResizeShortestEdge as RSE
    assert RSE.get_output_shape(480, 640, 800, 1333) == (800, 1067)
    assert RSE.get_output_shape(1024, 2048, 800, 1333) == (667, 1333)
    assert RSE.get_output_shape(1024, 2048, 1024, 2048) == (1024, 2048)
    assert RSE.get_output_shape(375, 500, 800, 1333) == (800, 1067)
    assert RSE((0,), 1333, "choice").get_params(48, 64, np.random.RandomState(0)) == (48, 64)             # size 0: no-op


def test_box_transform_directed_cases():
    from aldi_amd import aug
    p = aug.WeakParams(100, 200, 50, 100, flip=False)
    assert np.array_equal(aug.transform_boxes(np.array([[20.0, 10.0, 60.0, 30.0]]), p), [[10.0, 5.0, 30.0, 15.0]])
    pf = aug.WeakParams(100, 200, 50, 100, flip=True)
    assert np.array_equal(aug.transform_boxes(np.array([[20.0, 10.0, 60.0, 30.0]]), pf), [[70.0, 5.0, 90.0, 15.0]])     # x -> new_w - x, min / max
    # a box past the border is clipped to [0, W] x [0, H]
    assert np.array_equal(aug.transform_boxes(np.array([[-10.0, -4.0, 260.0, 120.0]]), p), [[0.0, 0.0, 100.0, 50.0]])
    # a box outside the image collapses on the border and is dropped with its class; the others keep their order
    inst = {"image_size": (100, 200), "gt_boxes": torch.tensor([[20.0, 10.0, 60.0, 30.0], [210.0, 10.0, 230.0, 30.0], [0.0, 0.0, 200.0, 100.0]]),
            "gt_classes": torch.tensor([3, 5, 7])}
    out = aug.transform_instances(inst, pf)
    assert out["image_size"] == (50, 100) and out["gt_boxes"].dtype == torch.float32
    assert torch.equal(out["gt_boxes"], torch.tensor([[70.0, 5.0, 90.0, 15.0], [0.0, 0.0, 100.0, 50.0]])) and out["gt_classes"].tolist() == [3, 7]
    assert inst["gt_boxes"].shape == (3, 4) and inst["image_size"] == (100, 200)                          # the record's own dict is untouched
    empty = aug.transform_instances({"image_size": (100, 200), "gt_boxes": torch.zeros(0, 4), "gt_classes": torch.zeros(0, dtype=torch.int64)}, pf)
    assert empty["gt_boxes"].shape == (0, 4) and empty["gt_classes"].shape == (0,)
    # float64 on the host, one cast at the end: 1/3 scales
    p3 = aug.WeakParams(3, 3, 1, 1, flip=True)
    exp = np.array([[1 - 2.0 * (1 * 1.0 / 3), 1.0 * (1 * 1.0 / 3), 1 - 1.0 * (1 * 1.0 / 3), 2.0 * (1 * 1.0 / 3)]])
    assert np.array_equal(aug.transform_boxes(np.array([[1.0, 1.0, 2.0, 2.0]]), p3), exp)


@pytest.mark.parametrize("style,sizes", [("choice", (64, 96, 80)), ("range", (64, 96))])
def test_draw_sequence_is_size_then_flip_per_image(style, sizes):
    from aldi_amd import aug
    augs = [aug.ResizeShortestEdge(sizes, 160, style), aug.RandomFlip(0.5, horizontal=True)]
    rs, ref = np.random.RandomState(11), np.random.RandomState(11)
    for h, w in [(96, 128), (128, 96), (50, 300), (96, 128)] * 3:
        p = aug.draw_weak_params(augs, h, w, rs)
        size = ref.choice(sizes) if style == "choice" else ref.randint(sizes[0], sizes[1] + 1)
        flip = ref.uniform(0, 1.0) < 0.5
        assert p == aug.WeakParams(h, w, *aug.ResizeShortestEdge.get_output_shape(h, w, int(size), 160), flip=bool(flip))
    assert np.array_equal(rs.get_state()[1], ref.get_state()[1]) and rs.get_state()[2] == ref.get_state()[2]
    # no flip stage: only the size is drawn
    rs, ref = np.random.RandomState(5), np.random.RandomState(5)
    p = aug.draw_weak_params(augs[:1], 96, 128, rs)
    ref.choice(sizes) if style == "choice" else ref.randint(sizes[0], sizes[1] + 1)
    assert not p.flip and rs.get_state()[2] == ref.get_state()[2] and np.array_equal(rs.get_state()[1], ref.get_state()[1])
    with pytest.raises(TypeError):
        aug.draw_weak_params(augs, 96, 128, np.random.default_rng(0))


def _cfg():
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    return cfg


def test_config_default_is_off_and_unsupported_geometry_is_rejected_by_name():
    from aldi_amd import aug
    cfg = _cfg()
    assert cfg.AUG.DEVICE_WEAK is False and cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING == "choice" and cfg.INPUT.RANDOM_FLIP == "horizontal"
    train, test = aug.get_weak_augs(cfg, True), aug.get_weak_augs(cfg, False)
    assert [type(a) for a in train] == [aug.ResizeShortestEdge, aug.RandomFlip] and [type(a) for a in test] == [aug.ResizeShortestEdge]
    assert train[0].short_edge_length == (800,) and train[0].max_size == 1333 and not train[0].is_range and train[1].prob == 0.5
    assert test[0].short_edge_length == (800, 800) and test[0].max_size == 1333
    cfg.INPUT.RANDOM_FLIP = "none"
    assert [type(a) for a in aug.get_weak_augs(cfg, True)] == [aug.ResizeShortestEdge]
    cfg.INPUT.RANDOM_FLIP = "vertical"
    with pytest.raises(ValueError, match="AUG.DEVICE_WEAK.*RANDOM_FLIP"):
        aug.get_weak_augs(cfg, True)
    cfg.INPUT.RANDOM_FLIP = "horizontal"
    cfg.INPUT.CROP.ENABLED = True
    with pytest.raises(ValueError, match="AUG.DEVICE_WEAK.*INPUT.CROP.ENABLED"):
        aug.get_weak_augs(cfg, True)
    # keys a user's YAML already set survive add_aldi_config
    from aldi_amd.config import add_aldi_config, get_cfg
    c2 = get_cfg()
    c2.INPUT.MIN_SIZE_TRAIN_SAMPLING = "range"
    c2.INPUT.RANDOM_FLIP = "none"
    add_aldi_config(c2)
    assert c2.INPUT.MIN_SIZE_TRAIN_SAMPLING == "range" and c2.INPUT.RANDOM_FLIP == "none"


def test_seeds_of_the_three_draw_streams_differ():
    from aldi_amd.dataloader import device_strong_seed, device_weak_seed
    seeds = {f(b, r, lab) for f in (device_strong_seed, device_weak_seed) for b in (0, 1) for r in (0, 1) for lab in (True, False)}
    assert len(seeds) == 16


def test_plan_follows_the_knob_and_the_row_window():
    """aldi_geom_plan (host only): fused when the knob is on and every 16-row tile's input rows fit ALDI_GEOM_LDS_ROWS"""
    import ctypes
    from aldi_amd import _lib as L
    from aldi_amd import aug

    def plan(h, new_h):
        f = ctypes.c_int(-1)
        yb = aug.resize_tables(h, new_h)[1] if h != new_h else None
        L.call("aldi_geom_plan", yb.ctypes.data if yb is not None else None, h, new_h, ctypes.byref(f))
        return f.value
    L.reset_tuning()
    try:
        assert plan(37, 80) == 1 and plan(64, 25) == 1 and plan(50, 50) == 1 and plan(240, 100) == 1
        assert plan(100, 7) == 0                                   # 7 output rows read all 100 input rows: more than 96
        assert plan(1024, 800) == 1 and plan(1024, 512) == 1
        L.set_tuning("resize_fused", 0)
        assert plan(37, 80) == 0 and plan(50, 50) == 0
    finally:
        L.reset_tuning()
    f = ctypes.c_int(0)
    assert L.lib.aldi_geom_plan(None, 10, 20, ctypes.byref(f)) == -2 and b"geom_plan" in L.lib.aldi_last_error()
    assert L.lib.aldi_geom_batch_resize(None, 1, None, 0, 0, 0, None) == -2 and b"geom_batch_resize" in L.lib.aldi_last_error()

"""Inference API, host side (aldi_amd/postprocess.py, tta.py, config.py, csrc/infer.hip's argument checks): the descriptor's one
rounding, the CPU restatements of tests/infer_refs.py against hand-computed cases, the order of the test-time views, the
TEST.AUG defaults, and ALDI_ERR_ARG from both entry points without a GPU."""
import ctypes

import numpy as np
import torch

import infer_refs as R

F = np.float32


def _cfg(*opts):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_list(list(opts))
    return cfg


def _fields(t):
    return {k: F(getattr(t, k)) for k in ("flip_w", "sx0", "sy0", "sx1", "sy1", "clip_w", "clip_h")}


def test_box_tfm_rounds_each_double_ratio_once_to_float32():
    from aldi_amd import _lib as L
    from aldi_amd.postprocess import box_tfm
    assert ctypes.sizeof(L.BoxTfm) == 32
    import re
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} aldi_box_tfm;", open(L.HEADER_PATH).read(), flags=re.S).group(1)
    names = [part.strip().split()[-1] for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in L.BoxTfm._fields_]                                  # the binding's field order is the header's
    t = box_tfm((1024, 640), (1024 / 800, 640 / 500))
    assert F(t.sx0) == F(1.28) and F(t.sy0) == F(1.28) and t.sx0 != 1.28              # the float32 nearest to 1.28, not the double
    assert (t.sx1, t.sy1, t.flip_w, t.clip_w, t.clip_h, t.pad) == (1.0, 1.0, -1.0, 1024.0, 640.0, 0)
    t = box_tfm((37, 53), (53 / 37, 37 / 53), (37 / 53, 53 / 37), flip_w=85)
    assert F(t.sx0) == F(53 / 37) and F(t.sy0) == F(37 / 53) and F(t.sx1) == F(37 / 53) and F(t.sy1) == F(53 / 37) and t.flip_w == 85.0
    assert t.sx0 != 53 / 37 and np.float64(t.sx0) == np.float64(F(53 / 37))           # one rounding: float32(double ratio)
    # not float32(53) / float32(37) rounded again, nor a product of rounded factors: the value is the double ratio's nearest float32
    assert abs(np.float64(t.sx0) - 53 / 37) <= np.spacing(F(53 / 37)) / 2
    assert _fields(t) == R.desc((37, 53), (53 / 37, 37 / 53), (37 / 53, 53 / 37), 85)


def test_view_tfm_is_flip_then_view_to_input_then_input_to_original():
    from aldi_amd.aug import WeakParams
    from aldi_amd.tta import view_tfm
    p = WeakParams(50, 70, 64, 90, True)
    assert _fields(view_tfm(p, 100, 140)) == R.view_desc(50, 70, 64, 90, True, 100, 140)
    t = view_tfm(WeakParams(50, 70, 64, 90, False), 50, 70)
    assert t.flip_w == -1.0 and (t.sx1, t.sy1) == (1.0, 1.0) and F(t.sx0) == F(70 / 90) and F(t.sy0) == F(50 / 64) and (t.clip_w, t.clip_h) == (70.0, 50.0)


def test_restated_transform_on_hand_computed_boxes():
    # flip at 100: [10, 20, 30, 60] -> x 90, 70; scale0 (0.5, 2): [45, 40, 35, 120]; scale1 (2, 1): [90, 40, 70, 120];
    # corners re-ordered: [70, 40, 90, 120]; clip (80, 100): [70, 40, 80, 100]
    d = R.desc((80, 100), (0.5, 2.0), (2.0, 1.0), 100)
    assert R.tfm_numpy([[10, 20, 30, 60]], d).tolist() == [[70.0, 40.0, 80.0, 100.0]]
    # no flip, scale 1: a no-op up to the clip; a box left of 0 collapses onto x = 0
    d1 = R.desc((50, 50))
    assert R.tfm_numpy([[-30, 5, -5, 20], [1.5, 2.5, 60, 70]], d1).tolist() == [[0.0, 5.0, 0.0, 20.0], [1.5, 2.5, 50.0, 50.0]]
    # the multiply is a float32 multiply by the rounded scale
    d2 = R.desc((4000, 4000), (1024 / 800, 1.0))
    assert R.tfm_numpy([[3, 0, 7, 1]], d2)[0, 0] == F(3) * F(1.28) and R.tfm_numpy([[3, 0, 7, 1]], d2)[0, 2] == F(7) * F(1.28)


def test_restated_postprocess_on_hand_computed_rows():
    boxes = torch.tensor([[[10, 10, 20, 20],        # kept: x 2, y 0.5 -> [20, 5, 40, 10]
                           [45, 10, 60, 20],        # x 90 .. 120 -> both clamp to 80: zero width, dropped
                           [-30, 10, -5, 20],       # left of 0: dropped
                           [12, 10, 12, 20],        # x1 == x2: dropped
                           [30, 190, 35, 230],      # y 95 .. 115 -> 95 .. 100: kept
                           [1, 1, 2, 2]]],          # past the count: ignored
                         dtype=torch.float32)
    scores = torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]])
    classes = torch.tensor([[0, 1, 2, 0, 1, 2]], dtype=torch.int32)
    ob, os_, oc, on = R.postprocess(boxes, scores, classes, [5], [R.desc((80, 100), (2.0, 0.5))])
    assert on.tolist() == [2]
    assert ob[0].tolist() == [[20, 5, 40, 10], [60, 95, 70, 100]] + [[0, 0, 0, 0]] * 4
    assert os_[0].tolist() == [F(0.9), 0.5, 0, 0, 0, 0] and oc[0].tolist() == [0, 1, -1, -1, -1, -1]
    ob, os_, oc, on = R.postprocess(boxes, scores, classes, [0], [R.desc((80, 100))])
    assert on.tolist() == [0] and not ob.any() and not os_.any() and (oc == -1).all()


def test_restated_merge_on_the_directed_case():
    boxes, scores, classes, count, exp = R.directed_merge_case()
    descs = [R.desc((100, 100))] * 3
    for topk in (100, 4):
        ob, os_, oc, n = R.merge(boxes, scores, classes, count, descs, 3, 1e-8, 0.5, topk)
        want = exp[:topk]
        assert n == len(want)
        assert ob[:n].tolist() == [[float(x) for x in r[0]] for r in want]
        assert os_[:n].tolist() == [float(F(r[1])) for r in want] and oc[:n].tolist() == [r[2] for r in want]
        assert not ob[n:].any() and not os_[n:].any() and (oc[n:] == -1).all()
    assert R.merge(boxes, scores, classes, np.zeros(3, np.int32), descs, 3, 1e-8, 0.5, 10)[3] == 0


def test_tta_view_order_and_shapes():
    from aldi_amd.aug import ResizeShortestEdge, WeakParams
    from aldi_amd.tta import tta_params
    cfg = _cfg("TEST.AUG.MIN_SIZES", (48, 64), "TEST.AUG.MAX_SIZE", 96)
    s48, s64 = ResizeShortestEdge.get_output_shape(50, 70, 48, 96), ResizeShortestEdge.get_output_shape(50, 70, 64, 96)
    assert s48 == (48, 67) and s64 == (64, 90)
    assert tta_params(cfg, 50, 70) == [WeakParams(50, 70, *s48, False), WeakParams(50, 70, *s48, True),
                                       WeakParams(50, 70, *s64, False), WeakParams(50, 70, *s64, True)]
    cfg.TEST.AUG.FLIP = False
    assert tta_params(cfg, 50, 70) == [WeakParams(50, 70, *s48, False), WeakParams(50, 70, *s64, False)]
    cfg.TEST.AUG.MAX_SIZE = 80                                                      # the long side is capped
    assert [(p.new_h, p.new_w) for p in tta_params(cfg, 50, 70)] == [(48, 67), ResizeShortestEdge.get_output_shape(50, 70, 64, 80)]
    state = np.random.get_state()[1].copy()
    tta_params(cfg, 50, 70)
    assert np.array_equal(np.random.get_state()[1], state)                           # no draw is consumed


def test_test_aug_defaults_are_detectron2s():
    cfg = _cfg()
    a = cfg.TEST.AUG
    assert a.ENABLED is False and tuple(a.MIN_SIZES) == (400, 500, 600, 700, 800, 900, 1000, 1100, 1200) and a.MAX_SIZE == 4000 and a.FLIP is True


def test_tta_wrapper_refuses_a_model_that_is_not_on_an_rcnn_engine():
    import pytest
    from aldi_amd.tta import GeneralizedRCNNWithTTA

    class Detr:
        detr = True

        def inference(self, *a, **k):
            return []
    with pytest.raises(TypeError):
        GeneralizedRCNNWithTTA(_cfg(), Detr())
    with pytest.raises(TypeError):
        GeneralizedRCNNWithTTA(_cfg(), object())


def test_entry_points_report_argument_errors_without_a_gpu():
    from aldi_amd import _lib as L
    one = ctypes.c_void_p(64)                              # never dereferenced: the checks return before any launch
    rc = L.lib.aldi_detector_postprocess(None, None, None, None, 1, 4, None, None, None, None, None, None)
    assert rc == -2 and b"null" in L.lib.aldi_last_error()
    rc = L.lib.aldi_detector_postprocess(one, one, one, one, 1, 4, None, one, one, one, one, None)      # (the descriptors alone missing)
    assert rc == -2 and b"null" in L.lib.aldi_last_error()
    rc = L.lib.aldi_tta_merge(None, None, None, None, None, 1, 2, 4, 3, 1e-8, 0.5, 10, None, None, None, None, None, None)
    assert rc == -2 and b"null" in L.lib.aldi_last_error()
    rc = L.lib.aldi_tta_merge(one, one, one, one, one, 1, 83, 100, 3, 1e-8, 0.5, 10, one, one, one, one, one, None)
    assert rc == -2 and b"8192" in L.lib.aldi_last_error()                                              # 8300 candidates
    assert L.lib.aldi_tta_merge_workspace(1, 83, 100) == 0 and L.lib.aldi_tta_merge_workspace(1, 81, 100) > 0
    assert L.lib.aldi_tta_merge_workspace(1, 8193, 1) == 0 and L.lib.aldi_tta_merge_workspace(1, 1, 8192) > 0     # the bound itself is accepted
    assert L.lib.aldi_tta_merge_workspace(2, 3, 5) >= 2 * 64 * (16 + 4 + 4 + 4 + 8 + 4)
    try:
        L.call("aldi_tta_merge", None, None, None, None, None, 1, 2, 4, 3, 1e-8, 0.5, 10, None, None, None, None, None, None)
        assert False
    except L.AldiHipError as e:
        assert "tta_merge" in str(e)

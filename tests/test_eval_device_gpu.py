"""COCO box AP on the device (aldi_amd/evaluation.py DeviceCOCOEvaluator, csrc/eval.hip, TEST.DEVICE_EVAL) against the host evaluator.

The requirement is EQUALITY, not a tolerance: both sides do the same correctly rounded fp64 operations on the same doubles, so
`precision`, `recall` and `valid` are compared with `np.array_equal` and the six summary numbers with `==` (NaN where the host
gives NaN).  The six numbers are also held against oracle/coco_eval.py to the abs=1e-9 that tests/test_evaluation_cpu.py uses."""
import copy
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """evaluators, trainers and their device buffers are collected here, at a quiet point with the device idle, rather than by a
    collection that happens to run inside a later test's step"""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()


def _inst(size, boxes, scores, classes, device="cuda"):
    from aldi_amd.structures import Boxes, Instances
    inst = Instances(size)
    inst.pred_boxes = Boxes(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).to(device))
    inst.scores = torch.as_tensor(scores, dtype=torch.float32).reshape(-1).to(device)
    inst.pred_classes = torch.as_tensor(classes, dtype=torch.int64).reshape(-1).to(device)
    return inst


def _feed_of(records, dets, net_size=None, device="cuda"):
    """one `process` call per image, as build_test_loader batches them"""
    feed = []
    for r, d in zip(records, dets):
        size = net_size or (r["height"], r["width"])
        feed.append(([dict(image_id=r["image_id"], height=r["height"], width=r["width"])], [_inst(size, d["boxes"], d["scores"], d["classes"], device)]))
    return feed


def _host_tables(adapter):
    """{(category, area index): accumulate(...)} exactly as coco_bbox_metrics forms them"""
    from collections import defaultdict
    from aldi_amd.evaluation import AREA_RNG, MAX_DETS, accumulate, evaluate_img, maybe_add_optional_annotations
    anns = [dict(a) for a in adapter.annotations]
    maybe_add_optional_annotations(anns)
    gts, dts = defaultdict(list), defaultdict(list)
    for a in anns:
        gts[a["image_id"], a["category_id"]].append(a)
    for d in adapter._predictions:
        dts[d["image_id"], d["category_id"]].append(d)
    ids = [im["id"] for im in adapter.images]
    return {(c, ai): accumulate([evaluate_img(dts.get((i, c), []), gts.get((i, c), []), rng, MAX_DETS[-1]) for i in ids])
            for c in range(adapter.num_classes) for ai, rng in enumerate(AREA_RNG.values())}


def _same(a, b):
    return a == b or (a != a and b != b)


def _compare(records, feed, K):
    """host adapter vs device evaluator on the same (inputs, Instances): tables equal, six numbers equal, oracle to 1e-9"""
    from aldi_amd.evaluation import AREA_RNG, DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter, maybe_add_optional_annotations
    from oracle import coco_eval as oc
    host = Detectron2COCOEvaluatorAdapter("val", records, K, distributed=False)
    dev = DeviceCOCOEvaluator("val", records, K, distributed=False)
    for inputs, outputs in feed:
        host.process(inputs, outputs)
        dev.process(inputs, outputs)
    rh, rd = host.evaluate()["bbox"], dev.evaluate()["bbox"]
    tables = _host_tables(host)
    for c in range(K):
        for ai in range(len(AREA_RNG)):
            t = tables[c, ai]
            assert int(dev.last["valid"][c, ai]) == (0 if t is None else 1), (c, ai)
            if t is not None:
                assert np.array_equal(dev.last["precision"][c, ai], t[0]), (c, ai, np.abs(dev.last["precision"][c, ai] - t[0]).max())
                assert np.array_equal(dev.last["recall"][c, ai], t[1]), (c, ai)
    print("host", dict(rh), "device", dict(rd))
    assert list(rd) == list(rh) == list(KEYS)
    for k in KEYS:
        assert _same(rd[k], rh[k]), (k, rd[k], rh[k])
    anns = copy.deepcopy(host.annotations)
    maybe_add_optional_annotations(anns)                             # the oracle expects `iscrowd` / `area` filled in
    ref = oc.bbox_metrics([im["id"] for im in host.images], anns, host._predictions, list(range(K)))
    for k, v in ref.items():
        assert (np.isnan(v) and np.isnan(rd[k])) or rd[k] == pytest.approx(v, abs=1e-9), (k, rd[k], v)
    return rh, rd, dev, host


def _random_scene(seed):
    """the generator of tests/test_evaluation_cpu.py::test_random_scenes_match_loop_oracle as records + per-image detections"""
    rng = np.random.RandomState(seed)
    records, dets = [], []
    for i in range(6):
        anns, d = [], []
        for _ in range(rng.randint(0, 6)):
            x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(8, 200), rng.uniform(8, 200)
            c = int(rng.randint(0, 3))
            anns.append(dict(bbox=[float(x), float(y), float(w), float(h)], bbox_mode="XYWH_ABS", category_id=c, area=float(w * h),
                             iscrowd=int(rng.rand() < 0.15)))
            if rng.rand() < 0.8:                                     # a jittered detection of it
                j = rng.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h])
                d.append((c if rng.rand() < 0.9 else int(rng.randint(0, 3)), (x + j[0], y + j[1], max(w + j[2], 2), max(h + j[3], 2)),
                          round(float(rng.rand()), 2)))               # rounded scores: ties exercise the stable sorts
        for _ in range(rng.randint(0, 4)):                           # clutter
            d.append((int(rng.randint(0, 3)), (rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(5, 150), rng.uniform(5, 150)),
                      round(float(rng.rand()), 2)))
        records.append(dict(image_id=i, height=600, width=600, annotations=anns))
        dets.append(dict(boxes=[[b[0], b[1], b[0] + b[2], b[1] + b[3]] for _, b, _ in d], scores=[s for _, _, s in d], classes=[c for c, _, _ in d]))
    return records, dets


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_scenes_equal_host(seed):
    records, dets = _random_scene(seed)
    _compare(records, _feed_of(records, dets), 3)


def test_large_scene_equal_host():
    """50 images of 2048 x 1024, 8 categories, 5-39 ground-truth boxes each (5 % crowd), exactly 100 detections per image"""
    from aldi_amd import synthetic as syn
    records, dets = syn.make_eval_scene(50, 8, 1024, 2048, seed=0)
    assert all(len(d["scores"]) == 100 for d in dets) and all(5 <= len(r["annotations"]) <= 39 for r in records)
    from aldi_amd.evaluation import Detectron2COCOEvaluatorAdapter
    feed = _feed_of(records, dets)
    host = Detectron2COCOEvaluatorAdapter("val", records, 8, distributed=False)
    for inputs, outputs in feed:
        host.process(inputs, outputs)
    rh = host.evaluate()["bbox"]
    assert all(np.isfinite(rh[k]) and 0.0 < rh[k] < 100.0 for k in KEYS), rh      # no comparison below is NaN against NaN
    _compare(records, feed, 8)


def _ann(box, cat, mode="XYWH_ABS", **kw):
    d = dict(bbox=[float(v) for v in box], bbox_mode=mode, category_id=cat)
    d.update(kw)
    return d


def _directed(name):
    """-> (records, detections per image, num_classes, network size or None)"""
    img = lambda i, anns, h=400, w=600: dict(image_id=i, height=h, width=w, annotations=anns)
    xyxy = lambda b: [b[0], b[1], b[0] + b[2], b[1] + b[3]]
    det = lambda rows: dict(boxes=[xyxy(b) for b, _, _ in rows], scores=[s for _, s, _ in rows], classes=[c for _, _, c in rows])
    if name == "duplicate_gt":              # equal IoU against two identical boxes: the later one is taken, the next detection gets the first
        a = [_ann((50, 50, 100, 80), 0, area=8000.0), _ann((50, 50, 100, 80), 0, area=8000.0), _ann((300, 200, 60, 60), 0, area=3600.0)]
        d = det([((52, 51, 100, 80), 0.9, 0), ((50, 50, 100, 80), 0.9, 0), ((300, 200, 60, 50), 0.7, 0)])
        return [img(0, a)], [d], 1, None
    if name == "crowd":                     # one detection inside a crowd box, then two more inside the same crowd box
        a = [_ann((20, 20, 100, 100), 0, area=10000.0), _ann((200, 100, 300, 250), 0, area=75000.0, iscrowd=1)]
        d = det([((20, 20, 100, 90), 0.95, 0), ((210, 110, 50, 50), 0.9, 0), ((220, 150, 60, 40), 0.8, 0), ((300, 200, 80, 80), 0.8, 0),
                 ((10, 300, 40, 40), 0.5, 0)])
        return [img(0, a)], [d], 1, None
    if name == "no_gt_and_no_dt":           # image 0: detections of category 1 without ground truth; image 1: ground truth without detections
        r = [img(0, [_ann((10, 10, 50, 50), 0, area=2500.0)]), img(1, [_ann((30, 30, 90, 120), 1, area=10800.0), _ann((200, 50, 40, 40), 0, area=1600.0)])]
        d = [det([((10, 10, 50, 50), 0.9, 0), ((100, 100, 60, 60), 0.8, 1), ((300, 100, 70, 30), 0.6, 1)]), det([((200, 50, 40, 44), 0.7, 0)])]
        return r, d, 2, None
    if name == "more_than_100":             # 130 detections of one category in one image: the stable cut to 100
        rng = np.random.RandomState(5)
        a = [_ann((20 + 55 * k, 30, 50, 60), 0, area=3000.0) for k in range(10)] + [_ann((20 + 55 * k, 200, 50, 60), 1, area=3000.0) for k in range(3)]
        rows = [((20 + 55 * (k % 10) + rng.uniform(-6, 6), 30 + rng.uniform(-6, 6), 50, 60), round(float(rng.uniform(0.05, 0.6)), 2), 0) for k in range(130)]
        rows += [((20 + 55 * k, 200, 50, 58), 0.5, 1) for k in range(3)]
        return [img(0, a)], [det(rows)], 2, None
    if name == "absent_category":           # category 2 has neither ground truth nor detections: valid == 0, left out of the mean
        a = [_ann((10, 10, 80, 80), 0, area=6400.0), _ann((200, 200, 120, 100), 1, area=12000.0)]
        d = det([((12, 10, 80, 80), 0.9, 0), ((200, 205, 120, 100), 0.8, 1), ((400, 50, 30, 30), 0.3, 1)])
        return [img(0, a)], [d], 3, None
    if name == "missing_area":              # no `area`: the reference's y * w; (150, 4, 100, 100) becomes "small" (400), (10, 300, 40, 20) "large" (12000)
        a = [_ann((150, 4, 100, 100), 0), _ann((10, 300, 40, 20), 0), _ann((300, 100, 50, 50), 0, iscrowd=0)]
        d = det([((150, 4, 100, 96), 0.9, 0), ((10, 300, 40, 20), 0.8, 0), ((300, 100, 50, 45), 0.7, 0), ((400, 300, 20, 20), 0.6, 0)])
        return [img(0, a)], [d], 1, None
    if name == "rescale_and_clip":          # original 400 x 600 seen at 200 x 300; two boxes clip to empty and are dropped, one is cut by the border
        a = [_ann((40, 20, 200, 100), 0, area=20000.0), _ann((500, 300, 100, 100), 0, area=10000.0)]
        d = dict(boxes=[[20.1, 10.3, 120.7, 60.2], [310.0, 50.0, 340.0, 80.0], [250.0, 150.0, 320.0, 230.0], [100.0, -30.0, 150.0, -5.0]],
                 scores=[0.9, 0.8, 0.7, 0.6], classes=[0, 0, 0, 0])
        return [img(0, a)], [d], 1, (200, 300)
    if name == "xyxy_records":              # ground truth given as XYXY_ABS (as build_test_loader's records are)
        a = [_ann((10.5, 20.25, 110.75, 90.5), 0, mode="XYXY_ABS"), _ann((200.1, 100.2, 333.3, 288.8), 1, mode="XYXY_ABS", iscrowd=0)]
        d = det([((10.5, 20.25, 100.0, 70.0), 0.9, 0), ((200.0, 100.0, 133.0, 188.0), 0.8, 1), ((50, 300, 60, 60), 0.4, 1)])
        return [img(0, a)], [d], 2, None
    if name == "many_gt":                   # 280 ground-truth boxes in one (image, category): past the register flags (64) and the LDS stage (256)
        rng = np.random.RandomState(11)
        cells = [(4 + 29 * (k % 20), 4 + 28 * (k // 20)) for k in range(280)]
        a = [_ann((x, y, 24, 22), 0, area=528.0, iscrowd=int(k % 37 == 5)) for k, (x, y) in enumerate(cells)]
        rows = [((cells[k][0] + rng.uniform(-3, 3), cells[k][1] + rng.uniform(-3, 3), 24, 22), round(float(rng.uniform(0.1, 0.9)), 2), 0)
                for k in rng.permutation(280)[:60]]
        return [img(0, a)], [det(rows)], 1, None
    raise KeyError(name)


DIRECTED = ["duplicate_gt", "crowd", "no_gt_and_no_dt", "more_than_100", "absent_category", "missing_area", "rescale_and_clip", "xyxy_records",
            "many_gt"]


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_cases_equal_host(name):
    records, dets, K, net = _directed(name)
    rh, rd, dev, host = _compare(records, _feed_of(records, dets, net), K)
    if name == "absent_category":
        assert not dev.last["valid"][2].any() and dev.last["valid"][:2, 0].all()
    if name == "more_than_100":
        assert sum(p["category_id"] == 0 for p in host._predictions) == 130
    if name == "rescale_and_clip":
        assert len(host._predictions) == 2                          # the boxes right of and above the image are dropped by nonempty()
    if name == "duplicate_gt":
        assert rh["AP50"] == pytest.approx(100.0)                    # three boxes, each found: the duplicates do not steal each other's match


def test_host_tensors_and_dict_outputs_are_accepted():
    """`process` uploads host Instances and unwraps {"instances": ...} as the adapter does"""
    records, dets = _random_scene(1)
    feed = [(i, [{"instances": o[0]}]) for i, o in _feed_of(records, dets, device="cpu")]
    _compare(records, feed, 3)


def test_adapter_equivalence_in_batches():
    """the same list of (inputs, Instances), several images per `process` call, a reset in between: equal `evaluate()` dicts"""
    from aldi_amd import synthetic as syn
    from aldi_amd.evaluation import DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
    records, dets = syn.make_eval_scene(12, 4, 300, 500, seed=3, dets_per_image=40)
    one = _feed_of(records, dets)
    feed = [([x for i, _ in one[k:k + 4] for x in i], [x for _, o in one[k:k + 4] for x in o]) for k in range(0, 12, 4)]
    host = Detectron2COCOEvaluatorAdapter("val", records, 4, distributed=False)
    dev = DeviceCOCOEvaluator("val", records, 4, distributed=False)
    dev.process(*feed[0])
    dev.reset()                                                     # what inference_on_dataset does first
    for inputs, outputs in feed:
        host.process(inputs, outputs)
        dev.process(inputs, outputs)
    rh, rd = host.evaluate(), dev.evaluate()
    assert list(rh) == list(rd) == ["bbox"]
    assert all(_same(rh["bbox"][k], rd["bbox"][k]) for k in KEYS), (rh, rd)


def test_trainer_test_equal_with_device_eval_on_and_off():
    """ALDITrainer.test on a small synthetic configuration: same weights, same validation split, TEST.DEVICE_EVAL on and off"""
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.evaluation import DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.AMP.ENABLED", True, "SEED", 1, "SYNTHETIC.HEIGHT", 160, "SYNTHETIC.WIDTH", 224,
                         "SYNTHETIC.VAL_IMAGES", 4, "SOLVER.FUSED_STEP", False, "SOLVER.STEP_GRAPH", False])
    random.seed(0)
    torch.manual_seed(1)
    tr = ALDITrainer(cfg)
    assert type(ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])) is Detectron2COCOEvaluatorAdapter
    off = ALDITrainer.test(cfg, tr.ema.model)
    cfg.merge_from_list(["TEST.DEVICE_EVAL", True])
    assert type(ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])) is DeviceCOCOEvaluator
    on = ALDITrainer.test(cfg, tr.ema.model)
    print("off", dict(off["bbox"]), "on", dict(on["bbox"]))
    assert list(on["bbox"]) == list(off["bbox"]) == list(KEYS)
    assert all(_same(on["bbox"][k], off["bbox"][k]) for k in KEYS), (on, off)


def test_no_host_sync_before_the_final_copy():
    """`process`, the post-processing, the sorts and both kernels run under torch's sync debug mode "error" (positive control: a
    deliberate .item() raises under it on this build) AND with Tensor.cpu / item / tolist / numpy patched to count calls (the mode is
    a prototype that does not see every synchronising call; positive control: a deliberate .item() is counted).  Only the final
    copy of precision / recall / valid waits for the device.  A build without the mode is checked by the counters alone."""
    from aldi_amd import synthetic as syn
    from aldi_amd.evaluation import DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
    records, dets = syn.make_eval_scene(10, 4, 300, 500, seed=4, dets_per_image=60)
    feed = _feed_of(records, dets)
    dev = DeviceCOCOEvaluator("val", records, 4, distributed=False)
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    calls = []
    saved = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    own = {n for n in saved if n in vars(torch.Tensor)}
    try:
        for n, f in saved.items():
            setattr(torch.Tensor, n, (lambda f, n: lambda self, *a, **k: (calls.append(n), f(self, *a, **k))[1])(f, n))
        probe.item()
        assert calls == ["item"]                                     # positive control of the counters
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                probe.item()
                mode_works = False
            except RuntimeError:
                mode_works = True                                    # positive control of the mode
            if not mode_works:
                torch.cuda.set_sync_debug_mode("default")
            del calls[:]
            for inputs, outputs in feed:
                dev.process(inputs, outputs)
            out = dev._evaluate_device(dev._compact())
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert calls == [], calls
    finally:
        for n, f in saved.items():                                   # back to exactly what was there (inherited methods are not re-bound)
            setattr(torch.Tensor, n, f) if n in own else delattr(torch.Tensor, n)
    print("sync check through patched Tensor.cpu / item / tolist / numpy" + (" and torch.cuda.set_sync_debug_mode('error')" if mode_works else " only"))
    host = Detectron2COCOEvaluatorAdapter("val", records, 4, distributed=False)
    for inputs, outputs in feed:
        host.process(inputs, outputs)
    rh = host.evaluate()["bbox"]
    dev.reset()
    for inputs, outputs in feed:
        dev.process(inputs, outputs)
    rd = dev.evaluate()["bbox"]
    assert all(_same(rh[k], rd[k]) for k in KEYS)
    n_prec = 4 * 4 * 10 * 101
    assert np.array_equal(out[:n_prec].cpu().numpy().reshape(4, 4, 10, 101), dev.last["precision"])    # the run under the mode gave the same table


def test_argument_errors_are_reported():
    import aldi_amd._lib as L
    assert L.lib.aldi_coco_match(None, None, None, None, None, None, 4, 0, None, None, 100, None, None, None, None, None) == -2
    assert b"coco_match" in L.lib.aldi_last_error()
    assert L.lib.aldi_coco_match(None, None, None, None, None, None, 4, 0, None, None, 1000, None, None, None, None, None) == -2
    assert L.lib.aldi_coco_accumulate(None, None, None, None, None, 0, 3, None, None, None, None, None) == -2
    assert b"coco_accumulate" in L.lib.aldi_last_error()
    assert L.lib.aldi_coco_postprocess(None, None, None, None, None, 5, 3, None, None, None, None) == -2

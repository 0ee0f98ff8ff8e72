"""Evaluation detail on the device (DeviceCOCOEvaluator(detail=True), csrc/eval.hip aldi_coco_accumulate_detail, TEST.EVAL_DETAIL)
against the host evaluator with detail on.

As in tests/test_eval_device_gpu.py the requirement is EQUALITY: the extra fields are integer counts and one fp64 division of the
same operands, so the tables in `last` are compared with `np.array_equal` and every summary key with `==` (NaN where the host
gives NaN).  What the host's numbers themselves are held against is in tests/test_eval_detail_cpu.py."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AP_KEYS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
AR_KEYS = ["AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
EXTRA = ("recall_at", "tp_thr", "fp_thr")


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """device buffers are collected here, at a quiet point with the device idle"""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()


def _inst(size, boxes, scores, classes):
    from aldi_amd.structures import Boxes, Instances
    inst = Instances(size)
    inst.pred_boxes = Boxes(torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).cuda())
    inst.scores = torch.as_tensor(scores, dtype=torch.float32).reshape(-1).cuda()
    inst.pred_classes = torch.as_tensor(classes, dtype=torch.int64).reshape(-1).cuda()
    return inst


def _feed_of(records, dets):
    """one `process` call per image, as build_test_loader batches them"""
    return [([dict(image_id=r["image_id"], height=r["height"], width=r["width"])], [_inst((r["height"], r["width"]), d["boxes"], d["scores"], d["classes"])])
            for r, d in zip(records, dets)]


def _host_tables(adapter, tau):
    """{(category, area index): (accumulate(...), accumulate_detail(...))} from the per-image results coco_bbox_metrics forms"""
    from collections import defaultdict
    from aldi_amd.evaluation import AREA_RNG, MAX_DETS, accumulate, accumulate_detail, evaluate_img, maybe_add_optional_annotations, score_cut
    anns = [dict(a) for a in adapter.annotations]
    maybe_add_optional_annotations(anns)
    gts, dts = defaultdict(list), defaultdict(list)
    for a in anns:
        gts[a["image_id"], a["category_id"]].append(a)
    for d in adapter._predictions:
        dts[d["image_id"], d["category_id"]].append(d)
    ids = [im["id"] for im in adapter.images]
    out = {}
    for c in range(adapter.num_classes):
        for ai, rng in enumerate(AREA_RNG.values()):
            per_img = [evaluate_img(dts.get((i, c), []), gts.get((i, c), []), rng, MAX_DETS[-1]) for i in ids]
            out[c, ai] = (accumulate(per_img), accumulate_detail(per_img, score_cut(tau)))
    return out


def _same(dev, host):
    return dev == host or (host != host and dev != dev)


def _compare(records, dets, K, tau, class_names=None):
    """host adapter vs device evaluator, detail on, the same (inputs, Instances): every table and every key equal"""
    from aldi_amd.evaluation import AREA_RNG, DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
    kw = dict(distributed=False, detail=True, score_thresh=tau, class_names=class_names)
    host, dev = Detectron2COCOEvaluatorAdapter("val", records, K, **kw), DeviceCOCOEvaluator("val", records, K, **kw)
    for inputs, outputs in _feed_of(records, dets):
        host.process(inputs, outputs)
        dev.process(inputs, outputs)
    rh, rd = host.evaluate()["bbox"], dev.evaluate()["bbox"]
    last = dev.last
    assert sorted(last) == sorted(("precision", "recall", "valid", "num_gt") + EXTRA)
    assert last["recall_at"].shape == (K, 4, 10, 2) and last["tp_thr"].shape == last["fp_thr"].shape == (K, 4, 10) and last["num_gt"].shape == (K, 4)
    for (c, ai), (t, d) in _host_tables(host, tau).items():
        assert int(last["valid"][c, ai]) == (0 if t is None else 1), (c, ai)
        if t is None:
            assert d is None and last["num_gt"][c, ai] == 0 and not any(last[k][c, ai].any() for k in EXTRA), (c, ai)
            continue
        assert np.array_equal(last["precision"][c, ai], t[0]) and np.array_equal(last["recall"][c, ai], t[1]), (c, ai)
        for k in EXTRA:
            assert np.array_equal(last[k][c, ai], d[k]), (k, c, ai, last[k][c, ai], d[k])
        assert last["num_gt"][c, ai] == d["num_gt"], (c, ai)
        assert np.array_equal(last["recall_at"][c, ai][:, 1] <= last["recall"][c, ai], np.ones(10, dtype=bool))
    print("host", dict(rh))
    print("device", dict(rd))
    assert list(rd) == list(rh) and list(rh)[:12] == AP_KEYS + AR_KEYS and len(rh) == 12 + 2 * K + (3 + 2 * K if tau is not None else 0)
    for k in rh:
        assert _same(rd[k], rh[k]), (k, rd[k], rh[k])
    return rh, rd, dev, host


def _ann(box, cat, **kw):
    d = dict(bbox=[float(v) for v in box], bbox_mode="XYWH_ABS", category_id=cat)
    d.update(kw)
    return d


def _img(i, anns, h=400, w=600):
    return dict(image_id=i, height=h, width=w, annotations=anns)


def _det(rows):
    """rows of (XYWH box, score, category)"""
    return dict(boxes=[[b[0], b[1], b[0] + b[2], b[1] + b[3]] for b, _, _ in rows], scores=[s for _, s, _ in rows], classes=[c for _, _, c in rows])


def _random_scene(seed):
    """the generator of tests/test_evaluation_cpu.py::test_random_scenes_match_loop_oracle as records + per-image detections"""
    rng = np.random.RandomState(seed)
    records, dets = [], []
    for i in range(6):
        anns, d = [], []
        for _ in range(rng.randint(0, 6)):
            x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(8, 200), rng.uniform(8, 200)
            c = int(rng.randint(0, 3))
            anns.append(_ann((x, y, w, h), c, area=float(w * h), iscrowd=int(rng.rand() < 0.15)))
            if rng.rand() < 0.8:
                j = rng.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h])
                d.append(((x + j[0], y + j[1], max(w + j[2], 2), max(h + j[3], 2)), round(float(rng.rand()), 2), c if rng.rand() < 0.9 else int(rng.randint(0, 3))))
        for _ in range(rng.randint(0, 4)):
            d.append(((rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(5, 150), rng.uniform(5, 150)), round(float(rng.rand()), 2), int(rng.randint(0, 3))))
        records.append(_img(i, anns, 600, 600))
        dets.append(_det(d))
    return records, dets


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_scenes_equal_host(seed):
    """6 images, K = 3, tau = 0.5; scores rounded to two decimals, so ties sit on the cut"""
    records, dets = _random_scene(seed)
    rh, _, _, _ = _compare(records, dets, 3, 0.5, class_names=["person", "car", "rider"] if seed == 1 else None)
    assert all(np.isfinite(rh[k]) for k in ("AR1", "AR10", "AR100", "Prec50", "Rec50")), rh          # not NaN against NaN
    assert rh["ScoreThr"] == 0.5 and (seed != 1 or "AP50-car" in rh)


GRID = [(10 + 48 * (k % 12), 10 + 60 * (k // 12), 40, 50) for k in range(24)]


def test_rank_edges_1_10_11_12_detections():
    """categories with 1, 10, 11 and 12 detections in one image, each matching a box of its own, in descending score order: the
    cut at 10 drops one match of the third category and two of the fourth; the cut at 1 keeps one match everywhere"""
    counts = (1, 10, 11, 12)
    anns = [_ann(GRID[k], c, area=2000.0) for c in range(4) for k in range(12)]
    rows = [(GRID[k], 0.99 - 0.01 * k - 0.001 * c, c) for c, n in enumerate(counts) for k in range(n)]
    rh, rd, dev, _ = _compare([_img(0, anns, 200, 600)], [_det(rows)], 4, 0.5)
    for c, n in enumerate(counts):
        assert np.array_equal(dev.last["recall_at"][c, 0], np.tile([1 / 12, min(n, 10) / 12], (10, 1))), c
        assert np.array_equal(dev.last["recall"][c, 0], np.full(10, n / 12))
    assert rd["AR1"] == pytest.approx(100.0 / 12) and rd["AR10"] == pytest.approx(100.0 * 31 / 48) and rd["AR100"] == pytest.approx(100.0 * 34 / 48)


def test_rank_of_tied_top_scores_follows_the_stable_order():
    """two detections tied at the top, only the second in input order matches: the first has rank 0, so AR1 = 0"""
    anns = [_ann(GRID[0], 0, area=2000.0)]
    rows = [(GRID[5], 0.9, 0), (GRID[0], 0.9, 0), (GRID[7], 0.4, 0)]
    rh, rd, dev, _ = _compare([_img(0, anns)], [_det(rows)], 1, 0.5)
    assert rd["AR1"] == 0.0 and rd["AR10"] == 100.0 and rd["Prec50"] == 50.0 and rd["Rec50"] == 100.0


def test_rank_is_per_image():
    """three images with one matching detection each (ranks 0, 0, 0 -- not 0, 1, 2 of the category's list): AR1 = 100"""
    records = [_img(i, [_ann(GRID[i], 0, area=2000.0)]) for i in range(3)]
    dets = [_det([(GRID[i], 0.9 - 0.2 * i, 0)]) for i in range(3)]
    rh, rd, dev, _ = _compare(records, dets, 1, 0.6)
    assert rd["AR1"] == 100.0 and rd["Rec50"] == pytest.approx(200.0 / 3) and rd["Prec50"] == 100.0


def _crowded(counts, seed, K=1):
    """images with counts[i] detections of category 0 around 12 ground-truth boxes, scores rounded to two decimals"""
    rng = np.random.RandomState(seed)
    records, dets = [], []
    for i, n in enumerate(counts):
        anns = [_ann(GRID[k], 0, area=2000.0) for k in range(12)]
        rows = [((GRID[k % 12][0] + rng.uniform(-8, 8), GRID[k % 12][1] + rng.uniform(-8, 8), 40, 50), round(float(rng.uniform(0.05, 0.95)), 2), 0) for k in range(n)]
        records.append(_img(i, anns, 200, 600))
        dets.append(_det(rows))
    return records, dets


def test_chunk_carry_337_detections():
    """one category, 337 kept detections over four images (100 + 100 + 100 + 37): more than one 256-element chunk of the walk and
    not a multiple of one, so the per-thread counters run over two rounds and the last chunk is partly empty"""
    records, dets = _crowded((100, 100, 100, 37), seed=7)
    rh, rd, dev, host = _compare(records, dets, 1, 0.5)
    assert len(host._predictions) == 337
    assert 0 < dev.last["tp_thr"][0, 0, 0] < dev.last["tp_thr"][0, 0, 0] + dev.last["fp_thr"][0, 0, 0] < 337 and 0 < rd["AR1"] < rd["AR10"] < rd["AR100"]


def test_130_detections_in_one_image_are_cut_before_the_ranks():
    """130 detections of one category in one image: the stable cut to 100 comes first, ranks and the counts above tau see 100"""
    records, dets = _crowded((130,), seed=5)
    rh, rd, dev, host = _compare(records, dets, 1, 0.05)
    assert len(host._predictions) == 130
    assert dev.last["tp_thr"][0, 0, 0] + dev.last["fp_thr"][0, 0, 0] <= 100


def test_crowd_detections_above_the_cut_are_neither_tp_nor_fp():
    """the `crowd` scene of tests/test_eval_device_gpu.py: three detections inside a crowd box are ignored"""
    a = [_ann((20, 20, 100, 100), 0, area=10000.0), _ann((200, 100, 300, 250), 0, area=75000.0, iscrowd=1)]
    d = _det([((20, 20, 100, 90), 0.95, 0), ((210, 110, 50, 50), 0.9, 0), ((220, 150, 60, 40), 0.8, 0), ((300, 200, 80, 80), 0.8, 0), ((10, 300, 40, 40), 0.5, 0)])
    rh, rd, dev, _ = _compare([_img(0, a)], [d], 1, 0.4)
    assert dev.last["tp_thr"][0, 0, 0] == 1 and dev.last["fp_thr"][0, 0, 0] == 1 and rd["Prec50"] == 50.0 and rd["Rec50"] == 100.0


def test_missing_area_scene():
    """the `missing_area` scene of tests/test_eval_device_gpu.py: areas from the reference's y * w move boxes between the ranges"""
    a = [_ann((150, 4, 100, 100), 0), _ann((10, 300, 40, 20), 0), _ann((300, 100, 50, 50), 0, iscrowd=0)]
    d = _det([((150, 4, 100, 96), 0.9, 0), ((10, 300, 40, 20), 0.8, 0), ((300, 100, 50, 45), 0.7, 0), ((400, 300, 20, 20), 0.6, 0)])
    _compare([_img(0, a)], [d], 1, 0.65)


def test_categories_without_ground_truth():
    """category 1 has detections only, category 2 neither ground truth nor detections: valid == 0, NaN per-category keys, and
    neither enters the AR means or the micro sums (the numbers are those of category 0 alone)"""
    a = [_ann(GRID[0], 0, area=2000.0), _ann(GRID[3], 0, area=2000.0)]
    rows = [(GRID[0], 0.9, 0), (GRID[8], 0.85, 0), (GRID[3], 0.6, 0), (GRID[5], 0.99, 1), (GRID[6], 0.95, 1)]
    rh, rd, dev, _ = _compare([_img(0, a)], [_det(rows)], 3, 0.8)
    assert not dev.last["valid"][1:].any() and dev.last["valid"][0].any()
    for c in (1, 2):
        assert all(np.isnan(rd["%s-%d" % (p, c)]) for p in ("AP", "AP50", "Prec50", "Rec50"))
    assert rd["AR1"] == 50.0 and rd["AR100"] == 100.0 and rd["Prec50"] == 50.0 and rd["Rec50"] == 50.0
    rows0 = [r for r in rows if r[2] == 0]
    r1, _, _, _ = _compare([_img(0, a)], [_det(rows0)], 1, 0.8)
    assert all(_same(rd[k], r1[k]) for k in AP_KEYS + AR_KEYS + ["Prec50", "Rec50"])


def test_tau_at_float32_0p8_with_scores_on_and_beside_it():
    """float32 scores at float32(0.8) and its neighbours: only the upper neighbour is above the cut (strict, in float32)"""
    t = np.float32(0.8)
    up, down = np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))
    anns = [_ann(GRID[k], 0, area=2000.0) for k in range(4)]
    rows = [(GRID[0], float(t), 0), (GRID[1], float(up), 0), (GRID[2], float(down), 0), (GRID[9], float(up), 0), (GRID[10], float(t), 0)]
    rh, rd, dev, _ = _compare([_img(0, anns)], [_det(rows)], 1, 0.8)
    assert dev.last["tp_thr"][0, 0, 0] == 1 and dev.last["fp_thr"][0, 0, 0] == 1
    assert rd["ScoreThr"] == float(t) and rd["Prec50"] == 50.0 and rd["Rec50"] == 25.0
    rh, rd, dev, _ = _compare([_img(0, anns)], [_det(rows)], 1, float(up))                    # nothing exceeds the upper neighbour
    assert np.isnan(rd["Prec50"]) and rd["Rec50"] == 0.0


def test_detail_without_a_score_cut_and_detail_off():
    """`score_thresh=None`: no keys at the cut, zero counts; `detail=False`: today's six keys, three tables and buffer"""
    from aldi_amd.evaluation import DeviceCOCOEvaluator
    records, dets = _random_scene(2)
    rh, rd, dev, _ = _compare(records, dets, 3, None)
    assert "ScoreThr" not in rd and not dev.last["tp_thr"].any() and not dev.last["fp_thr"].any()
    off = DeviceCOCOEvaluator("val", records, 3, distributed=False)
    for inputs, outputs in _feed_of(records, dets):
        off.process(inputs, outputs)
    assert off._evaluate_device(off._compact()).numel() == 3 * 4 * 10 * 101 + 3 * 4 * 10 + 6
    r0 = off.evaluate()["bbox"]
    assert list(r0) == AP_KEYS and sorted(off.last) == ["precision", "recall", "valid"]
    assert all(_same(r0[k], rd[k]) for k in AP_KEYS) and np.array_equal(off.last["precision"], dev.last["precision"])


def test_no_host_sync_before_the_final_copy_with_detail_on():
    """tests/test_eval_device_gpu.py's check with detail on: `process`, `_compact` and `_evaluate_device(..., detail=True)` under
    torch's sync debug mode "error" where the build has it and with Tensor.cpu / item / tolist / numpy counted (positive controls
    for both); nothing waits for the device before the final copy"""
    from aldi_amd import synthetic as syn
    from aldi_amd.evaluation import DeviceCOCOEvaluator
    records, dets = syn.make_eval_scene(10, 4, 300, 500, seed=4, dets_per_image=60)
    feed = _feed_of(records, dets)
    dev = DeviceCOCOEvaluator("val", records, 4, distributed=False, detail=True, score_thresh=0.5)
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
            out = dev._evaluate_device(dev._compact(), detail=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert calls == [], calls
    finally:
        for n, f in saved.items():                                   # back to exactly what was there
            setattr(torch.Tensor, n, f) if n in own else delattr(torch.Tensor, n)
    print("sync check through patched Tensor.cpu / item / tolist / numpy" + (" and torch.cuda.set_sync_debug_mode('error')" if mode_works else " only"))
    K, A, T, R = 4, 4, 10, 101
    assert out.numel() == K * A * T * R + K * A * T + K * A // 2 + 4 * K * A * T + K * A
    host = out.cpu().numpy()
    dev.reset()
    for inputs, outputs in feed:
        dev.process(inputs, outputs)
    rd = dev.evaluate()["bbox"]
    off = K * A * T * R + K * A * T + K * A // 2                     # the run under the mode gave the same fields, appended after `valid`
    assert np.array_equal(host[:K * A * T * R].reshape(K, A, T, R), dev.last["precision"])
    assert np.array_equal(host[off:off + 2 * K * A * T].reshape(K, A, T, 2), dev.last["recall_at"])
    assert np.array_equal(host[off + 2 * K * A * T:off + 3 * K * A * T].reshape(K, A, T), dev.last["tp_thr"])
    assert np.array_equal(host[off + 3 * K * A * T:off + 4 * K * A * T].reshape(K, A, T), dev.last["fp_thr"])
    assert np.array_equal(host[off + 4 * K * A * T:].reshape(K, A), dev.last["num_gt"])
    assert dev.last["tp_thr"][:, 0, 0].sum() > 0 and dev.last["fp_thr"][:, 0, 0].sum() > 0 and np.isfinite(rd["Prec50"])


def test_trainer_test_equal_with_device_eval_on_and_off_detail_on():
    """ALDITrainer.test on the small synthetic configuration of tests/test_eval_device_gpu.py with TEST.EVAL_DETAIL on"""
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.evaluation import DeviceCOCOEvaluator, Detectron2COCOEvaluatorAdapter
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SOLVER.AMP.ENABLED", True, "SEED", 1, "SYNTHETIC.HEIGHT", 160, "SYNTHETIC.WIDTH", 224,
                         "SYNTHETIC.VAL_IMAGES", 4, "SOLVER.FUSED_STEP", False, "SOLVER.STEP_GRAPH", False, "TEST.EVAL_DETAIL", True])
    assert cfg.DOMAIN_ADAPT.TEACHER.THRESHOLD == 0.8
    random.seed(0)
    torch.manual_seed(1)
    tr = ALDITrainer(cfg)
    ev = ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])
    assert type(ev) is Detectron2COCOEvaluatorAdapter and ev.detail and ev.score_thresh == 0.8
    off = ALDITrainer.test(cfg, tr.ema.model)
    cfg.merge_from_list(["TEST.DEVICE_EVAL", True])
    ev = ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])
    assert type(ev) is DeviceCOCOEvaluator and ev.detail and ev.score_thresh == 0.8
    on = ALDITrainer.test(cfg, tr.ema.model)
    print("off", dict(off["bbox"]))
    print("on", dict(on["bbox"]))
    K = ev.num_classes
    assert list(on["bbox"]) == list(off["bbox"]) and list(off["bbox"])[:12] == AP_KEYS + AR_KEYS and len(off["bbox"]) == 15 + 4 * K
    assert all(_same(on["bbox"][k], off["bbox"][k]) for k in off["bbox"]), (on, off)
    assert on["bbox"]["ScoreThr"] == float(np.float32(0.8)) and "AP50" in on["bbox"]


def test_argument_errors_are_reported():
    import aldi_amd._lib as L
    nul = [None] * 7
    assert L.lib.aldi_coco_accumulate_detail(*nul, 0, 3, None, 0.5, *nul, None) == -2
    assert b"coco_accumulate_detail" in L.lib.aldi_last_error()
    assert L.lib.aldi_coco_accumulate_detail(*nul, 4, 0, None, 0.5, *nul, None) == -2
    assert L.lib.aldi_coco_accumulate_detail(*nul, 4, 3, None, 0.5, *nul, None) == -2
    assert b"coco_accumulate_detail" in L.lib.aldi_last_error() and b"null" in L.lib.aldi_last_error()
    assert L.lib.aldi_coco_accumulate_detail(*nul, 4, 3, None, float("nan"), *nul, None) == -2
    assert b"coco_accumulate_detail" in L.lib.aldi_last_error() and b"NaN" in L.lib.aldi_last_error()

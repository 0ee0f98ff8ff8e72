"""Evaluation detail on the host (aldi_amd/evaluation.py: `detail`, `score_thresh`, `class_names`, `TEST.EVAL_DETAIL`): average
recall, per-category AP, and precision / recall of the detections above the teacher's score cut.

The per-category AP is held against oracle/coco_eval.py; AR and the numbers at the cut against a scalar loop written here (one
image, one detection, one threshold at a time, its own IoU -- it shares no code with evaluate_img / accumulate).  For the cut
the loop matches the FILTERED detections from scratch, which pins the argument that no re-matching is needed."""
import copy

import numpy as np
import pytest

AP_KEYS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
AR_KEYS = ["AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
THRS = [float(v) for v in np.linspace(0.5, 0.95, 10)]
AREAS = {"all": (0.0, 1e10), "small": (0.0, 32.0 ** 2), "medium": (32.0 ** 2, 96.0 ** 2), "large": (96.0 ** 2, 1e10)}


def _ann(img, cat, box, **kw):
    d = dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], area=float(box[2] * box[3]))
    d.update(kw)
    return d


def _det(img, cat, box, score):
    return dict(image_id=img, category_id=cat, bbox=[float(v) for v in box], score=float(score))


def _scene(seed):
    """the generator of tests/test_evaluation_cpu.py::test_random_scenes_match_loop_oracle"""
    rng = np.random.RandomState(seed)
    imgs = [dict(id=i) for i in range(6)]
    anns, dets = [], []
    for i in range(6):
        for _ in range(rng.randint(0, 6)):
            x, y, w, h = rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(8, 200), rng.uniform(8, 200)
            c = int(rng.randint(0, 3))
            anns.append(_ann(i, c, (x, y, w, h), iscrowd=int(rng.rand() < 0.15)))
            if rng.rand() < 0.8:
                j = rng.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h])
                dets.append(_det(i, c if rng.rand() < 0.9 else int(rng.randint(0, 3)), (x + j[0], y + j[1], max(w + j[2], 2), max(h + j[3], 2)),
                                 round(float(rng.rand()), 2)))
        for _ in range(rng.randint(0, 4)):
            dets.append(_det(i, int(rng.randint(0, 3)), (rng.uniform(0, 300), rng.uniform(0, 300), rng.uniform(5, 150), rng.uniform(5, 150)),
                             round(float(rng.rand()), 2)))
    return imgs, anns, dets


_RESULTS = {}


def _detail(seed, tau=0.5):
    """coco_bbox_metrics(detail=True) of a scene, computed once and shared (never modified)"""
    from aldi_amd.evaluation import coco_bbox_metrics
    if (seed, tau) not in _RESULTS:
        imgs, anns, dets = _scene(seed)
        _RESULTS[seed, tau] = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2], detail=True, score_thresh=tau)
    return _RESULTS[seed, tau]


def _loop_iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    return w * h / (d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - w * h)


def _loop_counts(imgs, anns, dets, cat, thr, area, max_det, tau=None):
    """-> (counted true positives, counted false positives, countable ground truth) of one category at one IoU threshold, area
    range and cut; with `tau` only the detections with float32(score) > float32(tau) exist at all"""
    tp = fp = n_gt = 0
    for im in imgs:
        gt = [a for a in anns if a["image_id"] == im["id"] and a["category_id"] == cat]
        dt = [d for d in dets if d["image_id"] == im["id"] and d["category_id"] == cat]
        if tau is not None:
            dt = [d for d in dt if np.float32(d["score"]) > np.float32(tau)]
        skip = [bool(a.get("iscrowd", 0)) or a["area"] < area[0] or a["area"] > area[1] for a in gt]
        n_gt += skip.count(False)
        gorder = [k for k in range(len(gt)) if not skip[k]] + [k for k in range(len(gt)) if skip[k]]
        used = set()
        for d in sorted(dt, key=lambda d: -d["score"])[:max_det]:
            best, hit = min(thr, 1 - 1e-10), None
            for k in gorder:
                crowd = bool(gt[k].get("iscrowd", 0))
                if k in used and not crowd:
                    continue
                if hit is not None and not skip[hit] and skip[k]:
                    break
                v = _loop_iou(d["bbox"], gt[k]["bbox"], crowd)
                if v >= best:
                    best, hit = v, k
            if hit is not None:
                used.add(hit)
                tp += not skip[hit]
            else:
                a = d["bbox"][2] * d["bbox"][3]
                fp += not (a < area[0] or a > area[1])
    return tp, fp, n_gt


def _loop_detail(imgs, anns, dets, cats, tau):
    out = {}
    for key, area, cut in (("AR1", "all", 1), ("AR10", "all", 10), ("AR100", "all", 100), ("ARs", "small", 100), ("ARm", "medium", 100),
                           ("ARl", "large", 100)):
        vals = []
        for c in cats:
            for t in THRS:
                tp, _, n = _loop_counts(imgs, anns, dets, c, t, AREAS[area], cut)
                if n:
                    vals.append(tp / n)
        out[key] = 100.0 * sum(vals) / len(vals) if vals else float("nan")
    stp = sfp = sn = 0
    for c in cats:
        tp, fp, n = _loop_counts(imgs, anns, dets, c, 0.5, AREAS["all"], 100, tau=tau)
        if n == 0:
            out["Prec50-%d" % c] = out["Rec50-%d" % c] = float("nan")
            continue
        stp, sfp, sn = stp + tp, sfp + fp, sn + n
        out["Prec50-%d" % c] = 100.0 * tp / (tp + fp) if tp + fp else float("nan")
        out["Rec50-%d" % c] = 100.0 * tp / n
    out["Prec50"] = 100.0 * stp / (stp + sfp) if stp + sfp else float("nan")
    out["Rec50"] = 100.0 * stp / sn if sn else float("nan")
    return out


def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == pytest.approx(b, abs=1e-9)


def test_detail_off_is_todays_dict_and_the_config_default_is_off():
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.evaluation import coco_bbox_metrics
    imgs, anns, dets = _scene(0)
    plain = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2])
    off = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2], detail=False, score_thresh=0.5, class_names=["a", "b", "c"])
    assert list(plain) == list(off) == AP_KEYS
    assert all(plain[k] == off[k] or (plain[k] != plain[k] and off[k] != off[k]) for k in AP_KEYS)
    on = _detail(0)
    assert all(plain[k] == on[k] or (plain[k] != plain[k] and on[k] != on[k]) for k in AP_KEYS)     # the six AP keys are unchanged
    cfg = get_cfg()
    add_aldi_config(cfg)
    assert cfg.TEST.EVAL_DETAIL is False


def test_key_order():
    from aldi_amd.evaluation import coco_bbox_metrics
    imgs, anns, dets = _scene(1)
    per = lambda names, *prefixes: [p + "-" + n for n in names for p in prefixes]
    res = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2], detail=True)
    assert list(res) == AP_KEYS + AR_KEYS + per("012", "AP", "AP50")
    res = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2], detail=True, score_thresh=0.5)
    assert list(res) == AP_KEYS + AR_KEYS + per("012", "AP", "AP50") + ["ScoreThr", "Prec50", "Rec50"] + per("012", "Prec50", "Rec50")
    names = ["person", "car", "traffic light"]
    named = coco_bbox_metrics(imgs, copy.deepcopy(anns), dets, [0, 1, 2], detail=True, score_thresh=0.5, class_names=names)
    assert list(named) == AP_KEYS + AR_KEYS + per(names, "AP", "AP50") + ["ScoreThr", "Prec50", "Rec50"] + per(names, "Prec50", "Rec50")
    assert list(named.values())[:12] == list(res.values())[:12] and named["AP-car"] == res["AP-1"] and named["Rec50-person"] == res["Rec50-0"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_per_category_ap_matches_loop_oracle(seed):
    from oracle import coco_eval as oc
    imgs, anns, dets = _scene(seed)
    res = _detail(seed)
    assert sum(np.isfinite(res["AP-%d" % c]) and np.isfinite(res["AP50-%d" % c]) for c in range(3)) >= 2, res
    ids = [im["id"] for im in imgs]
    for c in range(3):
        per = [oc.average_precision(ids, anns, dets, c, t) for t in THRS]
        want = float("nan") if per[0] is None else 100.0 * sum(per) / len(per)
        want50 = float("nan") if per[0] is None else 100.0 * per[0]
        assert _close(res["AP-%d" % c], want), (c, res["AP-%d" % c], want)
        assert _close(res["AP50-%d" % c], want50), (c, res["AP50-%d" % c], want50)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ar_and_cut_numbers_match_scalar_loop(seed):
    """tau = 0.5 with scores rounded to two decimals: ties sit on the cut"""
    imgs, anns, dets = _scene(seed)
    res = _detail(seed)
    ref = _loop_detail(imgs, anns, dets, [0, 1, 2], 0.5)
    assert all(np.isfinite(res[k]) for k in ("AR1", "AR10", "AR100", "Prec50", "Rec50")), res
    assert sum(np.isfinite(res["Prec50-%d" % c]) and np.isfinite(res["Rec50-%d" % c]) for c in range(3)) >= 2, res
    assert res["ScoreThr"] == 0.5
    for k, v in ref.items():
        assert _close(res[k], v), (k, res[k], v)
    assert res["AR1"] <= res["AR10"] <= res["AR100"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_flags_above_a_cut_do_not_depend_on_the_detections_below_it(seed):
    """evaluate_img of the detections above tau == the restriction of evaluate_img of all of them, in every (image, category, area)"""
    from aldi_amd.evaluation import AREA_RNG, evaluate_img
    imgs, anns, dets = _scene(seed)
    for a in anns:
        a.setdefault("iscrowd", 0)
    seen = 0
    for tau in (0.25, 0.5, 0.75):
        for im in imgs:
            for c in range(3):
                gt = [a for a in anns if a["image_id"] == im["id"] and a["category_id"] == c]
                dt = [d for d in dets if d["image_id"] == im["id"] and d["category_id"] == c]
                for rng in AREA_RNG.values():
                    full, part = evaluate_img(dt, gt, rng, 100), evaluate_img([d for d in dt if d["score"] > tau], gt, rng, 100)
                    if full is None:
                        assert part is None
                        continue
                    keep = full["scores"] > tau
                    if part is None:
                        assert not keep.any() and not gt
                        continue
                    seen += int(keep.sum())
                    assert np.array_equal(part["scores"], full["scores"][keep]) and part["num_gt"] == full["num_gt"]
                    assert np.array_equal(part["matched"], full["matched"][:, keep]) and np.array_equal(part["dt_ignore"], full["dt_ignore"][:, keep])
    assert seen > 20


def test_accumulate_max_det_and_recall_at_cut():
    from aldi_amd.evaluation import AREA_RNG, accumulate, evaluate_img, recall_at_cut
    imgs, anns, dets = _scene(2)
    for c in range(3):
        per_img = [evaluate_img([d for d in dets if d["image_id"] == im["id"] and d["category_id"] == c],
                                [a for a in anns if a["image_id"] == im["id"] and a["category_id"] == c], AREA_RNG["all"], 100) for im in imgs]
        full = accumulate(per_img)
        same = accumulate(per_img, max_det=None)
        assert np.array_equal(full[0], same[0]) and np.array_equal(full[1], same[1])
        assert np.array_equal(accumulate(per_img, max_det=100)[1], full[1])
        for m in (1, 2, 10):
            cut = accumulate(per_img, max_det=m)
            assert np.array_equal(recall_at_cut(per_img, m), cut[1])
            assert (cut[1] <= full[1]).all()
        # the cut is per image: what is left is the first column of each image, not of the concatenation
        assert sum(min(1, len(e["scores"])) for e in per_img if e is not None) > 1
    assert accumulate([None, None], max_det=1) is None and recall_at_cut([None], 1) is None


BOXES = [(10, 10, 50, 50), (100, 10, 60, 40), (200, 100, 80, 90)]


def _hand(scores, extra=(), tau=0.8):
    from aldi_amd.evaluation import coco_bbox_metrics
    anns = [_ann(0, 0, b) for b in BOXES]
    dets = [_det(0, 0, b, s) for b, s in zip(BOXES, scores)] + [_det(0, 0, b, s) for b, s in extra]
    return coco_bbox_metrics([dict(id=0)], anns, dets, [0], detail=True, score_thresh=tau)


def test_hand_case_three_boxes():
    res = _hand([0.9, 0.85, 0.5])
    assert res["AR1"] == pytest.approx(100.0 / 3, abs=1e-9) and res["AR10"] == pytest.approx(100.0) and res["AR100"] == pytest.approx(100.0)
    assert res["Prec50"] == pytest.approx(100.0) and res["Rec50"] == pytest.approx(200.0 / 3, abs=1e-9)
    assert res["Prec50-0"] == res["Prec50"] and res["Rec50-0"] == res["Rec50"] and res["ScoreThr"] == float(np.float32(0.8))
    assert res["AP-0"] == res["AP"] and res["AP50-0"] == res["AP50"] == pytest.approx(100.0)


def test_hand_case_clutter_on_top():
    res = _hand([0.9, 0.85, 0.5], extra=[((400, 300, 30, 30), 0.95)])
    assert res["AR1"] == 0.0 and res["AR10"] == pytest.approx(100.0) and res["AR100"] == pytest.approx(100.0)
    assert res["Prec50"] == pytest.approx(200.0 / 3, abs=1e-9) and res["Rec50"] == pytest.approx(200.0 / 3, abs=1e-9)


def test_the_cut_is_a_strict_float32_comparison():
    """scores at float32(0.8) and its float32 neighbours: only the upper neighbour is above tau = 0.8 (as a double, float32(0.8) is
    itself greater than 0.8, so a comparison in doubles against the unrounded tau would count it too)"""
    t = np.float32(0.8)
    up, down = np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0))
    assert float(down) < 0.8 < float(t) < float(up)
    res = _hand([float(t), float(up), float(down)])
    assert res["Prec50"] == pytest.approx(100.0) and res["Rec50"] == pytest.approx(100.0 / 3, abs=1e-9)
    res = _hand([float(t), float(down), float(down)])
    assert np.isnan(res["Prec50"]) and res["Rec50"] == 0.0
    res = _hand([float(up), float(up), float(down)], extra=[((400, 300, 30, 30), float(up)), ((300, 300, 30, 30), float(t))])
    assert res["Prec50"] == pytest.approx(200.0 / 3, abs=1e-9) and res["Rec50"] == pytest.approx(200.0 / 3, abs=1e-9)


def test_a_cut_nothing_exceeds():
    res = _hand([0.9, 0.85, 0.5], tau=0.95)
    assert np.isnan(res["Prec50"]) and res["Rec50"] == 0.0 and np.isnan(res["Prec50-0"]) and res["Rec50-0"] == 0.0
    assert res["AR100"] == pytest.approx(100.0)


def test_categories_without_ground_truth_are_left_out():
    """category 1 has detections only, category 2 nothing: NaN per-category keys, and neither moves a mean or a micro sum"""
    from aldi_amd.evaluation import coco_bbox_metrics
    anns = [_ann(0, 0, b) for b in BOXES]
    dets = [_det(0, 0, b, s) for b, s in zip(BOXES, [0.9, 0.85, 0.5])] + [_det(0, 1, (300, 300, 40, 40), 0.99)]
    res = coco_bbox_metrics([dict(id=0)], anns, dets, [0, 1, 2], detail=True, score_thresh=0.8)
    one = _hand([0.9, 0.85, 0.5])
    for k in AP_KEYS + AR_KEYS + ["Prec50", "Rec50"]:
        assert res[k] == one[k] or (res[k] != res[k] and one[k] != one[k]), k
    for c in (1, 2):
        assert all(np.isnan(res["%s-%d" % (p, c)]) for p in ("AP", "AP50", "Prec50", "Rec50"))


def test_adapter_and_trainer_pass_the_settings_on():
    import torch
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.evaluation import Detectron2COCOEvaluatorAdapter
    from aldi_amd.structures import Boxes, Instances
    from aldi_amd.trainer import ALDITrainer
    recs = [dict(image_id=7, height=200, width=400, annotations=[dict(bbox=[40, 20, 200, 100], bbox_mode="XYWH_ABS", category_id=1)])]
    inst = Instances((100, 200))
    inst.pred_boxes, inst.scores, inst.pred_classes = Boxes(torch.tensor([[20.0, 10.0, 120.0, 60.0]])), torch.tensor([0.9]), torch.tensor([1])
    plain = Detectron2COCOEvaluatorAdapter("toy_val", recs, num_classes=2, distributed=False)
    ev = Detectron2COCOEvaluatorAdapter("toy_val", recs, num_classes=2, distributed=False, detail=True, score_thresh=0.8, class_names=["a", "b"])
    for e in (plain, ev):
        e.process([dict(image_id=7, height=200, width=400)], [inst])
    assert list(plain.evaluate()["bbox"]) == AP_KEYS
    res = ev.evaluate()["bbox"]
    assert res["AR1"] == pytest.approx(100.0) and res["AP-b"] == pytest.approx(100.0) and np.isnan(res["AP-a"]) and res["Prec50-b"] == pytest.approx(100.0)
    cfg = get_cfg()
    add_aldi_config(cfg)
    off = ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])
    assert off.detail is False and off.score_thresh is None
    cfg.merge_from_list(["TEST.EVAL_DETAIL", True, "DOMAIN_ADAPT.TEACHER.THRESHOLD", 0.7])
    on = ALDITrainer.build_evaluator(cfg, "synthetic_val", dataset_dicts=[])
    assert type(on) is Detectron2COCOEvaluatorAdapter and on.detail is True and on.score_thresh == 0.7

"""COCO box-AP evaluation of a (teacher) model -- the host-side step after the hot path.

Mirrors what the reference reaches through `aldi/trainer.py:166-196`: `build_evaluator` -> `Detectron2COCOEvaluatorAdapter`
(`aldi/helpers.py:65-81`, a detectron2 `COCOEvaluator` that fills in missing `iscrowd` / `area`), `test()` on the EMA model, and
the `bbox/AP50` key `BestCheckpointer` watches.  detectron2 and pycocotools are not vendored in the reference tree (and absent
from this image), so the metric is a restatement of pycocotools' published `COCOeval` algorithm for iouType="bbox"
(evaluateImg greedy matching, accumulate's 101-point interpolated precision, summarize's 12 numbers: the six AP by default, the
six AR with `detail`, `TEST.EVAL_DETAIL`); it is cross-checked
against an independent loop implementation in oracle/coco_eval.py and hand-computed cases -- "parity unpinned" against
pycocotools itself.

Detections are consumed as the engine produces them (boxes in network-input pixels, XYXY) and mapped back to the original
image size like detectron2's `detector_postprocess` (scale by original/network size, clip).
"""
from __future__ import annotations

from collections import OrderedDict, defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = OrderedDict([("all", (0.0, 1e10)), ("small", (0.0, 32.0 ** 2)), ("medium", (32.0 ** 2, 96.0 ** 2)), ("large", (96.0 ** 2, 1e10))])


def maybe_add_optional_annotations(annotations: List[dict]) -> None:
    """reference aldi/helpers.py:65-70, verbatim semantics (including `area = bbox[1] * bbox[2]`, i.e. y * w, for annotations
    that carry no area -- kept so that numbers are comparable with the reference's logs)"""
    for ann in annotations:
        if "iscrowd" not in ann:
            ann["iscrowd"] = 0
        if "area" not in ann:
            ann["area"] = ann["bbox"][1] * ann["bbox"][2]


def iou_xywh(d: np.ndarray, g: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """(D, 4) x (G, 4) XYWH -> (D, G); against a crowd box the union is the detection's own area (maskUtils.iou)"""
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    dx2, dy2 = d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]
    gx2, gy2 = g[:, 0] + g[:, 2], g[:, 1] + g[:, 3]
    iw = np.clip(np.minimum(dx2[:, None], gx2[None]) - np.maximum(d[:, None, 0], g[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(dy2[:, None], gy2[None]) - np.maximum(d[:, None, 1], g[None, :, 1]), 0, None)
    inter = iw * ih
    da, ga = d[:, 2] * d[:, 3], g[:, 2] * g[:, 3]
    union = np.where(crowd[None], da[:, None], da[:, None] + ga[None] - inter)
    return inter / union


def evaluate_img(dt: List[dict], gt: List[dict], area_rng, max_det: int):
    """COCOeval.evaluateImg for one (image, category): -> dict(scores, matched [T, D], dt_ignore [T, D], num_gt) or None"""
    if not dt and not gt:
        return None
    g_ignore = np.array([bool(g.get("ignore", 0)) or bool(g["iscrowd"]) or g["area"] < area_rng[0] or g["area"] > area_rng[1] for g in gt], dtype=bool)
    gorder = np.argsort(g_ignore, kind="mergesort")                       # non-ignored ground truth first
    gt = [gt[i] for i in gorder]
    g_ignore = g_ignore[gorder]
    dorder = np.argsort([-d["score"] for d in dt], kind="mergesort")[:max_det]
    dt = [dt[i] for i in dorder]
    crowd = np.array([bool(g["iscrowd"]) for g in gt], dtype=bool)
    ious = iou_xywh(np.array([d["bbox"] for d in dt], dtype=np.float64).reshape(-1, 4),
                    np.array([g["bbox"] for g in gt], dtype=np.float64).reshape(-1, 4), crowd)
    T, D, G = len(IOU_THRS), len(dt), len(gt)
    dtm = -np.ones((T, D), dtype=np.int64)
    gtm = -np.ones((T, G), dtype=np.int64)
    dt_ig = np.zeros((T, D), dtype=bool)
    for ti, t in enumerate(IOU_THRS):
        for di in range(D):
            best, m = min(t, 1 - 1e-10), -1
            for gi in range(G):
                if gtm[ti, gi] >= 0 and not crowd[gi]:
                    continue                                    # already matched (a crowd box can absorb many detections)
                if m > -1 and not g_ignore[m] and g_ignore[gi]:
                    break                                       # matched a regular gt; the rest are ignore boxes
                if ious[di, gi] < best:
                    continue
                best, m = ious[di, gi], gi
            if m == -1:
                continue
            dt_ig[ti, di] = g_ignore[m]
            dtm[ti, di] = m
            gtm[ti, m] = di
    d_area = np.array([d["bbox"][2] * d["bbox"][3] for d in dt], dtype=np.float64)
    out_rng = (d_area < area_rng[0]) | (d_area > area_rng[1])
    dt_ig = dt_ig | ((dtm < 0) & out_rng[None])
    return dict(scores=np.array([d["score"] for d in dt], dtype=np.float64), matched=dtm >= 0, dt_ignore=dt_ig, num_gt=int((~g_ignore).sum()))


def _evaluated(per_img: List[Optional[dict]], max_det: Optional[int] = None):
    """the images that were evaluated, each cut to its first `max_det` detections (COCOeval's `[:, 0:maxDet]`; None: no cut
    beyond the one `evaluate_img` made), and their regular ground truth: -> (list, npig), or None where accumulate has no table"""
    ev = [e for e in per_img if e is not None]
    if not ev:
        return None
    npig = sum(e["num_gt"] for e in ev)
    if npig == 0:
        return None
    if max_det is not None:
        ev = [dict(e, scores=e["scores"][:max_det], matched=e["matched"][:, :max_det], dt_ignore=e["dt_ignore"][:, :max_det]) for e in ev]
    return ev, npig


def accumulate(per_img: List[Optional[dict]], max_det: Optional[int] = None):
    """COCOeval.accumulate for one (category, area range, maxDet): -> (precision [T, R], recall [T]) or None without gt.
    `max_det=m` keeps the first m detections of every image before they are concatenated."""
    cut = _evaluated(per_img, max_det)
    if cut is None:
        return None
    ev, npig = cut
    scores = np.concatenate([e["scores"] for e in ev])
    order = np.argsort(-scores, kind="mergesort")
    matched = np.concatenate([e["matched"] for e in ev], axis=1)[:, order]
    ignore = np.concatenate([e["dt_ignore"] for e in ev], axis=1)[:, order]
    tps = np.cumsum(matched & ~ignore, axis=1).astype(np.float64)
    fps = np.cumsum(~matched & ~ignore, axis=1).astype(np.float64)
    T, R = len(IOU_THRS), len(REC_THRS)
    precision = np.zeros((T, R))
    recall = np.zeros(T)
    for ti in range(T):
        tp, fp = tps[ti], fps[ti]
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        recall[ti] = rc[-1] if nd else 0.0
        pr = pr.tolist()
        for i in range(nd - 1, 0, -1):                           # precision envelope
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        inds = np.searchsorted(rc, REC_THRS, side="left")
        q = np.zeros(R)
        for ri, pi in enumerate(inds):
            if pi < nd:
                q[ri] = pr[pi]
        precision[ti] = q
    return precision, recall


def recall_at_cut(per_img: List[Optional[dict]], max_det: int):
    """`accumulate(per_img, max_det)[1]` without the precision table (average recall needs the recall vector only): the last
    element of a row of `tps` is the row's count, so this is the same integer over the same `npig`.  -> recall [T] or None"""
    cut = _evaluated(per_img, max_det)
    if cut is None:
        return None
    ev, npig = cut
    matched = np.concatenate([e["matched"] for e in ev], axis=1)
    ignore = np.concatenate([e["dt_ignore"] for e in ev], axis=1)
    tp = np.sum(matched & ~ignore, axis=1).astype(np.float64)
    return tp / npig if matched.shape[1] else np.zeros(len(IOU_THRS))


def score_cut(score_thresh) -> float:
    """tau as the comparison sees it: scores are float32 values held as doubles and `process_bbox` / `aldi_detections` compare in
    float32, so `np.float32(score) > np.float32(tau)` is `score > float(np.float32(tau))`.  None: a cut nothing exceeds."""
    if score_thresh is None:
        return float("inf")
    tau = float(np.float32(score_thresh))
    if tau != tau:
        raise ValueError("score_thresh is NaN")
    return tau


def counts_above(per_img: List[Optional[dict]], tau: float):
    """counted (not ignored) matched / unmatched detections with score > tau: -> (tp [T], fp [T]) as doubles, or None without gt.
    Nothing is matched again: COCO's greedy matching takes the detections in descending score order, so the flags of those
    above a cut do not depend on those below it (tests/test_eval_detail_cpu.py matches the filtered list from scratch)."""
    cut = _evaluated(per_img)
    if cut is None:
        return None
    ev, _ = cut
    above = np.concatenate([e["scores"] for e in ev]) > tau
    matched = np.concatenate([e["matched"] for e in ev], axis=1)
    ignore = np.concatenate([e["dt_ignore"] for e in ev], axis=1)
    return (np.sum(matched & ~ignore & above[None], axis=1).astype(np.float64), np.sum(~matched & ~ignore & above[None], axis=1).astype(np.float64))


def accumulate_detail(per_img: List[Optional[dict]], tau: float):
    """what the detail keys of `summarize_bbox` read besides (precision, recall), for one (category, area range):
    dict(recall_at [T, 2] at the cuts MAX_DETS[:2], tp_thr [T], fp_thr [T] above tau, num_gt) or None without gt"""
    cut = _evaluated(per_img)
    if cut is None:
        return None
    tp, fp = counts_above(per_img, tau)
    return dict(recall_at=np.stack([recall_at_cut(per_img, m) for m in MAX_DETS[:2]], axis=1), tp_thr=tp, fp_thr=fp, num_gt=float(cut[1]))


def coco_bbox_metrics(images: Sequence[dict], annotations: List[dict], detections: List[dict], category_ids: Sequence[int], detail: bool = False,
                      score_thresh: Optional[float] = None, class_names: Optional[Sequence[str]] = None) -> "OrderedDict[str, float]":
    """images: dict(id); annotations: dict(image_id, category_id, bbox XYWH[, iscrowd, area, ignore]); detections:
    dict(image_id, category_id, bbox XYWH, score) -> detectron2's `bbox` result dict (AP, AP50, AP75, APs, APm, APl in percent);
    `detail`: the further keys `summarize_bbox` lists"""
    maybe_add_optional_annotations(annotations)
    gts, dts = defaultdict(list), defaultdict(list)
    for a in annotations:
        gts[a["image_id"], a["category_id"]].append(a)
    for d in detections:
        dts[d["image_id"], d["category_id"]].append(d)
    img_ids = [im["id"] for im in images]
    prec: Dict[tuple, Optional[tuple]] = {}
    for c in category_ids:
        for an, rng in AREA_RNG.items():
            per_img = [evaluate_img(dts.get((i, c), []), gts.get((i, c), []), rng, MAX_DETS[-1]) for i in img_ids]
            prec[c, an] = accumulate(per_img)
            if detail and prec[c, an] is not None:
                prec[c, an] += (accumulate_detail(per_img, score_cut(score_thresh)),)
    return summarize_bbox(prec, category_ids, detail=detail, score_thresh=score_thresh, class_names=class_names)


def summarize_bbox(prec: Dict[tuple, Optional[tuple]], category_ids: Sequence[int], detail: bool = False, score_thresh: Optional[float] = None,
                   class_names: Optional[Sequence[str]] = None) -> "OrderedDict[str, float]":
    """COCOeval.summarize's six box AP numbers from {(category, area name): (precision [T, R], recall [T]) or None}.

    `detail=True` (the tables then carry a third element, `accumulate_detail`'s dict) appends, in this order:
    * AR1, AR10, AR100, ARs, ARm, ARl: COCOeval.summarize's six average-recall numbers -- 100 x the mean of recall[T] over the
      ten IoU thresholds and the categories that have a table (NaN without one); area `all` at the cuts 1 / 10 / 100, then the
      three area ranges at the cut 100;
    * per category c in index order, named class_names[c] or str(c): `AP-<name>`, detectron2's per-category AP (100 x the mean of
      the category's precision[T, R], area `all`; NaN without a table), and `AP50-<name>`, the same at IoU 0.5 -- an extension
      of ours, detectron2 has no such key;
    * with `score_thresh` (tau; DOMAIN_ADAPT.TEACHER.THRESHOLD in the trainer), the quality of the detections the pseudo labeler
      keeps, at IoU 0.5, area `all`, 100 detections per image: `ScoreThr` = float(np.float32(tau)); `Prec50` = 100 x sum(TP) /
      sum(TP + FP) and `Rec50` = 100 x sum(TP) / sum(npig), micro-averaged over the categories that have a table; then per
      category `Prec50-<name>` = 100 x TP_c / (TP_c + FP_c) (NaN when nothing is above the cut or there is no table) and
      `Rec50-<name>` = 100 x TP_c / npig_c.  TP_c / FP_c are the counted (not ignored) matched / unmatched detections of c with
      np.float32(score) > np.float32(tau), npig_c the category's countable ground truth.  Categories without countable
      ground truth are left out, as they are for AP: false positives of a class that is absent from the validation set are
      NOT seen by Prec50 / Rec50."""
    def summarize(area="all", iou=None):
        vals = []
        for c in category_ids:
            r = prec[c, area]
            if r is None:
                continue
            p = r[0]
            if iou is not None:
                p = p[np.isclose(IOU_THRS, iou)]
            vals.append(p)
        if not vals:
            return float("nan")
        return float(np.mean(np.stack(vals))) * 100.0
    res = OrderedDict([("AP", summarize()), ("AP50", summarize(iou=0.5)), ("AP75", summarize(iou=0.75)), ("APs", summarize("small")),
                       ("APm", summarize("medium")), ("APl", summarize("large"))])
    if not detail:
        return res
    nan = float("nan")

    def mean_recall(area="all", cut=None):
        vals = [prec[c, area][1] if cut is None else prec[c, area][2]["recall_at"][:, MAX_DETS.index(cut)] for c in category_ids
                if prec[c, area] is not None]
        return float(np.mean(np.stack(vals))) * 100.0 if vals else nan
    res.update([("AR1", mean_recall(cut=1)), ("AR10", mean_recall(cut=10)), ("AR100", mean_recall()), ("ARs", mean_recall("small")),
                ("ARm", mean_recall("medium")), ("ARl", mean_recall("large"))])
    names = [str(class_names[c]) if class_names is not None else str(c) for c in category_ids]
    t50 = int(np.flatnonzero(np.isclose(IOU_THRS, 0.5))[0])
    for c, name in zip(category_ids, names):
        r = prec[c, "all"]
        res["AP-" + name] = nan if r is None else float(np.mean(r[0])) * 100.0
        res["AP50-" + name] = nan if r is None else float(np.mean(r[0][t50])) * 100.0
    if score_thresh is None:
        return res
    counts = [None if prec[c, "all"] is None else tuple(float(prec[c, "all"][2][k][t50]) for k in ("tp_thr", "fp_thr")) + (float(prec[c, "all"][2]["num_gt"]),)
              for c in category_ids]
    tp, fp, npig = (sum(v[k] for v in counts if v is not None) for k in range(3))
    res["ScoreThr"] = score_cut(score_thresh)
    res["Prec50"] = 100.0 * tp / (tp + fp) if tp + fp > 0 else nan
    res["Rec50"] = 100.0 * tp / npig if npig > 0 else nan
    for v, name in zip(counts, names):
        res["Prec50-" + name] = 100.0 * v[0] / (v[0] + v[1]) if v is not None and v[0] + v[1] > 0 else nan
        res["Rec50-" + name] = 100.0 * v[0] / v[2] if v is not None else nan
    return res


class Detectron2COCOEvaluatorAdapter:
    """reset / process / evaluate with detectron2 COCOEvaluator's shapes (reference aldi/helpers.py:72-81).  `dataset_dicts`:
    detectron2-format records (file_name?, image_id, height, width, annotations=[dict(bbox XYWH_ABS or XYXY_ABS, bbox_mode,
    category_id[, iscrowd, area])]); contiguous category ids 0..K-1.  `detail` / `score_thresh` / `class_names` (`TEST.EVAL_DETAIL`):
    the further keys of `summarize_bbox` -- average recall, per-category AP, precision / recall above the score cut."""

    def __init__(self, dataset_name: str, dataset_dicts: Sequence[dict], num_classes: int, output_dir: Optional[str] = None,
                 distributed: bool = True, detail: bool = False, score_thresh: Optional[float] = None, class_names: Optional[Sequence[str]] = None):
        self.dataset_name, self.output_dir, self.distributed = dataset_name, output_dir, distributed
        self.num_classes = num_classes
        self.detail, self.score_thresh, self.class_names = bool(detail), score_thresh, class_names
        self.images = [dict(id=r["image_id"], height=r["height"], width=r["width"]) for r in dataset_dicts]
        self.annotations = []
        for r in dataset_dicts:
            for a in r.get("annotations", []):
                x, y, w, h = a["bbox"]
                if a.get("bbox_mode", "XYWH_ABS") in ("XYXY_ABS", 0):
                    w, h = w - x, h - y
                ann = dict(image_id=r["image_id"], category_id=a["category_id"], bbox=[float(x), float(y), float(w), float(h)])
                for k in ("iscrowd", "area"):
                    if k in a:
                        ann[k] = a[k]
                self.annotations.append(ann)
        self.reset()

    def reset(self):
        self._predictions: List[dict] = []

    def process(self, inputs: Sequence[dict], outputs: Sequence) -> None:
        """inputs: dict(image_id, height, width) of the ORIGINAL image; outputs: Instances (pred_boxes XYXY in network-input
        pixels, scores, pred_classes, image_size) as `GeneralizedRCNN.inference` returns them, or {"instances": Instances}"""
        for inp, out in zip(inputs, outputs):
            inst = out["instances"] if isinstance(out, dict) else out
            boxes = inst.pred_boxes.tensor.detach().float().cpu().numpy().reshape(-1, 4).astype(np.float64)
            ih, iw = inst.image_size
            sx, sy = inp["width"] / iw, inp["height"] / ih                      # detector_postprocess: back to the original size
            boxes[:, 0::2] = np.clip(boxes[:, 0::2] * sx, 0, inp["width"])
            boxes[:, 1::2] = np.clip(boxes[:, 1::2] * sy, 0, inp["height"])
            scores = inst.scores.detach().float().cpu().numpy()
            classes = inst.pred_classes.detach().cpu().numpy()
            keep = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])    # nonempty()
            for b, s, c in zip(boxes[keep], scores[keep], classes[keep]):
                self._predictions.append(dict(image_id=inp["image_id"], category_id=int(c), score=float(s),
                                              bbox=[float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]))

    def evaluate(self) -> "OrderedDict[str, dict]":
        preds = self._predictions
        if self.distributed:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                gathered = [None] * dist.get_world_size()
                dist.all_gather_object(gathered, preds)
                preds = [p for part in gathered for p in part]
                if dist.get_rank() != 0:
                    return OrderedDict()
        res = coco_bbox_metrics(self.images, [dict(a) for a in self.annotations], preds, list(range(self.num_classes)), detail=self.detail,
                                score_thresh=self.score_thresh, class_names=self.class_names)
        return OrderedDict(bbox=res)


def kernel_constants() -> Dict[str, np.ndarray]:
    """what the device kernels are handed: the host's own doubles (area_rng [4, 2], iou_thrs [10], rec_thrs [101])"""
    return dict(area_rng=np.array([r for r in AREA_RNG.values()], dtype=np.float64), iou_thrs=np.ascontiguousarray(IOU_THRS, dtype=np.float64),
                rec_thrs=np.ascontiguousarray(REC_THRS, dtype=np.float64))


def pack_ground_truth(images: Sequence[dict], annotations: List[dict], num_classes: int) -> Dict[str, np.ndarray]:
    """The adapter's annotation list per (image, category) segment `image_index * num_classes + category` (CSR, annotation order
    kept inside a segment): boxes [G, 4] XYWH, area [G] (after `maybe_add_optional_annotations`), flags [G] (bit 0 iscrowd,
    bit 1 ignore), off [I * K + 1].  Annotations of an unknown image or category are never looked up by the host and are dropped."""
    anns = [dict(a) for a in annotations]
    maybe_add_optional_annotations(anns)
    index = {}
    for i, im in enumerate(images):
        if im["id"] in index:
            raise ValueError(f"image id {im['id']!r} occurs twice")
        index[im["id"]] = i
    K, nseg = num_classes, len(images) * num_classes
    seg, rows = [], []
    for a in anns:
        c = a["category_id"]
        if a["image_id"] in index and c in range(K):
            seg.append(index[a["image_id"]] * K + int(c))
            rows.append(a)
    seg = np.array(seg, dtype=np.int64)
    order = np.argsort(seg, kind="mergesort")
    rows = [rows[i] for i in order]
    return dict(boxes=np.array([a["bbox"] for a in rows], dtype=np.float64).reshape(-1, 4),
                area=np.array([a["area"] for a in rows], dtype=np.float64),
                flags=np.array([(1 if a["iscrowd"] else 0) | (2 if a.get("ignore", 0) else 0) for a in rows], dtype=np.uint8),
                off=np.searchsorted(seg[order], np.arange(nseg + 1)).astype(np.int32))


def merge_detection_shards(shards: Sequence[tuple]) -> tuple:
    """Per-rank compact detections (boxes [n, 4] f64 XYWH, scores [n] f64, classes [n] i64, image index [n] i64, valid [n] bool),
    in any gather order -> one set keyed by image: ordered by image index, each image's detections in the order its rank
    produced them (what an unsharded run over the images in order holds)."""
    import torch
    cat = [torch.cat([s[k] for s in shards]) for k in range(5)]
    order = torch.sort(cat[3], stable=True)[1]
    return tuple(t[order] for t in cat)


class DeviceCOCOEvaluator:
    """`Detectron2COCOEvaluatorAdapter`'s interface and numbers with detections, matching and accumulation on the device
    (csrc/eval.hip; `TEST.DEVICE_EVAL`).  `process` appends to a device arena and launches nothing that waits for the device;
    `evaluate` runs the kernels and makes ONE device -> host copy (precision, recall, valid), which `summarize_bbox` turns into
    the six numbers with the host's numpy expressions.  With `detail` the accumulation kernel also counts what the further keys
    are made of (`aldi_coco_accumulate_detail`); the counts ride in the same buffer and the same copy, and the same
    `summarize_bbox` forms the keys."""

    def __init__(self, dataset_name: str, dataset_dicts: Sequence[dict], num_classes: int, output_dir: Optional[str] = None,
                 distributed: bool = True, device=None, detail: bool = False, score_thresh: Optional[float] = None,
                 class_names: Optional[Sequence[str]] = None):
        import torch
        from . import _lib as L
        host = Detectron2COCOEvaluatorAdapter(dataset_name, dataset_dicts, num_classes, output_dir=output_dir, distributed=distributed)
        self.dataset_name, self.output_dir, self.distributed, self.num_classes = dataset_name, output_dir, distributed, num_classes
        self.detail, self.score_thresh, self.class_names = bool(detail), score_thresh, class_names
        self.images, self.annotations = host.images, host.annotations         # converted exactly as the adapter converts them
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._index = {im["id"]: i for i, im in enumerate(self.images)}
        self._gt_host = pack_ground_truth(self.images, self.annotations, num_classes)
        self._gt = {k: self._upload(v) for k, v in self._gt_host.items()}
        self._const = {k: self._upload(v) for k, v in kernel_constants().items()}
        nseg = len(self.images) * num_classes
        self._seg_bounds = torch.arange(nseg + 2, device=self.device)
        self._cat_bounds = torch.arange(num_classes + 1, device=self.device)
        self._ws = torch.empty(int(L.lib.aldi_coco_match_workspace(len(self._gt_host["area"]))), dtype=torch.uint8, device=self.device)
        self._dummy = torch.zeros(64, dtype=torch.uint8, device=self.device)
        self._cap = 0
        self.last = None
        self.reset()

    def _upload(self, a: np.ndarray):
        """host array -> device through pinned memory (an asynchronous copy: nothing waits for the device)"""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a))
        return t.pin_memory().to(self.device, non_blocking=True) if t.numel() else torch.empty(t.shape, dtype=t.dtype, device=self.device)

    def _ptr(self, t):
        return t.data_ptr() if t.numel() else self._dummy.data_ptr()

    def reset(self):
        self._n = 0
        self._entries: List[tuple] = []          # per `process` entry: (sx, sy, width, height), image index, detections
        self._entry_img: List[int] = []
        self._entry_n: List[int] = []

    def _reserve(self, n: int):
        import torch
        if self._n + n <= self._cap:
            return
        cap = max(2 * self._cap, self._n + n, 4096)
        new = (torch.empty((cap, 4), dtype=torch.float32, device=self.device), torch.empty(cap, dtype=torch.float32, device=self.device),
               torch.empty(cap, dtype=torch.int64, device=self.device))
        if self._n:
            for dst, src in zip(new, (self._boxes, self._scores, self._classes)):
                dst[:self._n].copy_(src[:self._n])
        self._boxes, self._scores, self._classes = new
        self._cap = cap

    def process(self, inputs: Sequence[dict], outputs: Sequence) -> None:
        """as the adapter's `process`; the tensors stay on (or are uploaded to) the device, their lengths are host integers"""
        for inp, out in zip(inputs, outputs):
            inst = out["instances"] if isinstance(out, dict) else out
            boxes = inst.pred_boxes.tensor.detach().float().reshape(-1, 4)
            n = int(boxes.shape[0])
            ih, iw = inst.image_size
            self._entries.append((inp["width"] / iw, inp["height"] / ih, float(inp["width"]), float(inp["height"])))
            self._entry_img.append(self._index.get(inp["image_id"], -1))
            self._entry_n.append(n)
            if n == 0:
                continue
            self._reserve(n)
            s = slice(self._n, self._n + n)
            self._boxes[s].copy_(boxes, non_blocking=True)
            self._scores[s].copy_(inst.scores.detach().float().reshape(-1), non_blocking=True)
            self._classes[s].copy_(inst.pred_classes.detach().reshape(-1), non_blocking=True)
            self._n += n

    def _compact(self):
        """the arena through `aldi_coco_postprocess` -> (boxes XYWH f64, scores f64, classes, image index, valid)"""
        import torch
        from . import _lib as L, ops
        n = self._n
        counts = np.array(self._entry_n, dtype=np.int64)
        entry = self._upload(np.repeat(np.arange(len(counts), dtype=np.int32), counts))
        img = self._upload(np.repeat(np.array(self._entry_img, dtype=np.int64), counts))
        meta = self._upload(np.array(self._entries, dtype=np.float64).reshape(-1, 4))
        boxes = torch.empty((n, 4), dtype=torch.float64, device=self.device)
        scores = torch.empty(n, dtype=torch.float64, device=self.device)
        valid = torch.empty(n, dtype=torch.uint8, device=self.device)
        classes = self._classes[:n] if n else torch.empty(0, dtype=torch.int64, device=self.device)
        if n:
            with torch.cuda.device(self.device):
                L.call("aldi_coco_postprocess", self._boxes.data_ptr(), self._scores.data_ptr(), self._classes.data_ptr(), entry.data_ptr(),
                       meta.data_ptr(), n, self.num_classes, boxes.data_ptr(), scores.data_ptr(), valid.data_ptr(), ops.stream_ptr())
        return boxes, scores, classes, img, (valid != 0) & (img >= 0)

    def _layout(self, detail: bool) -> "OrderedDict[str, tuple]":
        """{field: (offset, length)} in doubles of the buffer `_evaluate_device` returns; the detail fields follow `valid`"""
        K, A, T, R = self.num_classes, len(AREA_RNG), len(IOU_THRS), len(REC_THRS)
        sizes = [("precision", K * A * T * R), ("recall", K * A * T), ("valid", (K * A + 1) // 2)]
        if detail:
            sizes += [("recall_at", K * A * T * 2), ("tp_thr", K * A * T), ("fp_thr", K * A * T), ("num_gt", K * A)]
        lay, off = OrderedDict(), 0
        for k, n in sizes:
            lay[k] = (off, n)
            off += n
        return lay

    def _evaluate_device(self, arrays, mark=lambda stage: None, detail: Optional[bool] = None):
        """match + accumulate -> one device buffer [precision K*4*10*101 | recall K*4*10 | valid K*4 (int32)]; no host sync.
        `detail` (None: the evaluator's own setting) appends [recall_at K*4*10*2 | tp_thr K*4*10 | fp_thr K*4*10 | num_gt K*4].
        `mark(stage)` is called after each stage has been enqueued (tools/bench_eval.py records device events there)."""
        import torch
        from . import _lib as L, ops
        boxes, scores, classes, img, valid = arrays
        detail = self.detail if detail is None else bool(detail)
        I, K, N = len(self.images), self.num_classes, int(scores.shape[0])
        nseg = I * K
        A = len(AREA_RNG)
        lay = self._layout(detail)
        n_prec, n_rec = lay["precision"][1], lay["recall"][1]
        out = torch.zeros(sum(n for _, n in lay.values()), dtype=torch.float64, device=self.device)
        if nseg == 0:
            return out
        # (image, category) segments, each in stable descending score order; invalid slots go to a bucket past the last segment
        key = torch.where(valid, img * K + classes, nseg)
        o1 = torch.sort(scores, descending=True, stable=True)[1]
        ks, o2 = torch.sort(key[o1], stable=True)
        order = o1[o2]
        sboxes, sscores = boxes[order].contiguous(), scores[order]
        det_off = torch.searchsorted(ks, self._seg_bounds).to(torch.int32)
        mark("segment_sorts")
        mbits = torch.zeros(N, dtype=torch.int64, device=self.device)
        igbits = torch.zeros(N, dtype=torch.int64, device=self.device)
        num_gt = torch.empty(nseg * A, dtype=torch.int32, device=self.device)
        g, c = self._gt, self._const
        with torch.cuda.device(self.device):
            L.call("aldi_coco_match", self._ptr(sboxes), det_off.data_ptr(), self._ptr(g["boxes"]), self._ptr(g["area"]), self._ptr(g["flags"]),
                   g["off"].data_ptr(), nseg, int(g["area"].shape[0]), c["area_rng"].data_ptr(), c["iou_thrs"].data_ptr(), MAX_DETS[-1],
                   self._ws.data_ptr(), self._ptr(mbits), self._ptr(igbits), num_gt.data_ptr(), ops.stream_ptr())
        mark("match")
        # per category: the slots that survived the cut, images in order, then the stable descending score order
        rank = torch.arange(N, device=self.device) - det_off[ks].long()
        key2 = torch.where((rank < MAX_DETS[-1]) & (ks < nseg), ks % K, K)
        p1 = torch.sort(sscores, descending=True, stable=True)[1]
        k2s, p2 = torch.sort(key2[p1], stable=True)
        perm = p1[p2].contiguous()
        cat_off = torch.searchsorted(k2s, self._cat_bounds).to(torch.int32)
        mark("category_sorts")
        with torch.cuda.device(self.device):
            if detail:      # the same walk also counts by rank (the tensor above, indexed through perm) and by score against tau
                L.call("aldi_coco_accumulate_detail", self._ptr(perm), cat_off.data_ptr(), self._ptr(mbits), self._ptr(igbits), num_gt.data_ptr(),
                       self._ptr(rank), self._ptr(sscores), I, K, c["rec_thrs"].data_ptr(), score_cut(self.score_thresh), out.data_ptr(),
                       *(out[lay[k][0]:].data_ptr() for k in ("recall", "valid", "recall_at", "tp_thr", "fp_thr", "num_gt")), ops.stream_ptr())
            else:
                L.call("aldi_coco_accumulate", self._ptr(perm), cat_off.data_ptr(), self._ptr(mbits), self._ptr(igbits), num_gt.data_ptr(), I, K,
                       c["rec_thrs"].data_ptr(), out.data_ptr(), out[n_prec:].data_ptr(), out[n_prec + n_rec:].data_ptr(), ops.stream_ptr())
        mark("accumulate")
        return out

    def evaluate(self) -> "OrderedDict[str, dict]":
        import torch
        arrays = self._compact()
        if self.distributed:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                gathered = [None] * dist.get_world_size()
                dist.all_gather_object(gathered, tuple(t.cpu() for t in arrays))       # one collective, as the adapter's list
                if dist.get_rank() != 0:
                    return OrderedDict()
                arrays = tuple(self._upload(t.numpy()) for t in merge_detection_shards(gathered))
        host = self._evaluate_device(arrays).cpu()                                       # the one device -> host copy
        K, A, T, R = self.num_classes, len(AREA_RNG), len(IOU_THRS), len(REC_THRS)
        lay = self._layout(self.detail)
        field = lambda k: host[lay[k][0]:lay[k][0] + lay[k][1]]
        precision = field("precision").numpy().reshape(K, A, T, R)
        recall = field("recall").numpy().reshape(K, A, T)
        valid = field("valid").view(torch.int32)[:K * A].numpy().reshape(K, A)
        self.last = dict(precision=precision, recall=recall, valid=valid)
        if self.detail:
            self.last.update(recall_at=field("recall_at").numpy().reshape(K, A, T, 2), tp_thr=field("tp_thr").numpy().reshape(K, A, T),
                             fp_thr=field("fp_thr").numpy().reshape(K, A, T), num_gt=field("num_gt").numpy().reshape(K, A))

        def table(c, ai):
            if not valid[c, ai]:
                return None
            more = (dict(recall_at=self.last["recall_at"][c, ai], tp_thr=self.last["tp_thr"][c, ai], fp_thr=self.last["fp_thr"][c, ai],
                         num_gt=float(self.last["num_gt"][c, ai])),) if self.detail else ()
            return (precision[c, ai], recall[c, ai]) + more
        prec = {(c, an): table(c, ai) for c in range(K) for ai, an in enumerate(AREA_RNG)}
        return OrderedDict(bbox=summarize_bbox(prec, list(range(K)), detail=self.detail, score_thresh=self.score_thresh, class_names=self.class_names))


def inference_on_dataset(model, data_loader, evaluator) -> "OrderedDict[str, dict]":
    """detectron2.evaluation.inference_on_dataset: eval-mode forward over the loader, evaluator.process per batch"""
    was_training = getattr(model, "training", False)
    model.eval()
    evaluator.reset()
    try:
        for inputs in data_loader:
            outputs = model(inputs)
            evaluator.process(inputs, outputs)
    finally:
        model.train(was_training)
    return evaluator.evaluate()

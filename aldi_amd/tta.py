"""Test-time augmentation for the R-CNN detectors (detectron2 `DatasetMapperTTA` + `GeneralizedRCNNWithTTA`, boxes only;
PARITY UNPINNED).  The views are made on the device by `aug.weak_views`; their detections are brought back to the original
image and merged class-wise by ONE `aldi_tta_merge` call per input (csrc/infer.hip)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from . import _lib as L
from . import aug, ops
from .postprocess import box_tfm, upload_tfms
from .structures import Boxes, Instances

SCORE_FLOOR = 1e-8      # GeneralizedRCNNWithTTA._merge_detections: fast_rcnn_inference_single_image(..., 1e-8, nms_thresh, topk)


def tta_params(cfg, h: int, w: int) -> List[aug.WeakParams]:
    """the views of an h x w image in `DatasetMapperTTA`'s order: for each of TEST.AUG.MIN_SIZES the unflipped view
    ResizeShortestEdge(min_size, TEST.AUG.MAX_SIZE), then the flipped one when TEST.AUG.FLIP"""
    out = []
    for m in cfg.TEST.AUG.MIN_SIZES:
        nh, nw = aug.ResizeShortestEdge.get_output_shape(h, w, int(m), int(cfg.TEST.AUG.MAX_SIZE))
        out.append(aug.WeakParams(h, w, nh, nw, False))
        if cfg.TEST.AUG.FLIP:
            out.append(aug.WeakParams(h, w, nh, nw, True))
    return out


def view_tfm(p: aug.WeakParams, height: int, width: int) -> L.BoxTfm:
    """a view's detections back to the (height, width) original: un-flip with the view's width, view -> input image, input
    image -> original, clip to (width, height)"""
    return box_tfm((width, height), (p.w / p.new_w, p.h / p.new_h), (width / p.w, height / p.h), flip_w=p.new_w if p.flip else None)


def tta_views(cfg, image: torch.Tensor, height: int, width: int) -> Tuple[List[Dict], List[L.BoxTfm]]:
    """`image`: an input dict's "image", uint8 (3, h, w) on the device; (height, width): the original image's size.
    -> (the views' input dicts {"image", "height", "width", "transforms": WeakParams}, one `aldi_box_tfm` per view).

    No random numbers are consumed: every size and every flip is fixed by the config.  (detectron2 runs the views through
    `apply_augmentations`, which consumes two draws per view from the global generator without using them.)"""
    if not (torch.is_tensor(image) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[0] == 3):
        raise ValueError("tta_views: the image must be uint8 of shape (3, h, w)")
    params = tta_params(cfg, int(image.shape[1]), int(image.shape[2]))
    src = image.to(cfg.MODEL.DEVICE).contiguous()
    outs = aug.weak_views([src] * len(params), params, chw_out=True, chw_in=True)
    views = [{"image": o, "height": int(height), "width": int(width), "transforms": p} for o, p in zip(outs, params)]
    return views, [view_tfm(p, int(height), int(width)) for p in params]


class GeneralizedRCNNWithTTA:
    """detectron2's wrapper of the same name for box detectors: `__call__(batched_inputs)` -> [{"instances": Instances}] in the
    original image's coordinates, `image_size = (height, width)`.  Per input: the views in view order, in groups of `batch_size`,
    through `model.inference(do_postprocess=False)`, then one `aldi_tta_merge` call (score floor 1e-8, MODEL.ROI_HEADS.NMS_THRESH_TEST,
    TEST.DETECTIONS_PER_IMAGE).  A view the engine cannot take (more than 512K anchors per image) raises in the engine, by name."""

    def __init__(self, cfg, model, batch_size: int = 3):
        if getattr(model, "detr", False) or not hasattr(model, "inference"):
            raise TypeError(f"GeneralizedRCNNWithTTA takes a model on an R-CNN engine, not {type(model).__name__}")
        if batch_size < 1:
            raise ValueError("GeneralizedRCNNWithTTA: batch_size must be positive")
        self.cfg, self.model, self.batch_size = cfg, model, int(batch_size)
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.topk = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        self.training = False

    # the surface `inference_on_dataset` uses
    def eval(self):
        self.model.eval()
        return self

    def train(self, mode: bool = True):
        self.model.train(mode)
        return self

    def __call__(self, batched_inputs: Sequence[Dict]) -> List[Dict]:
        with torch.no_grad():
            return [self._one(x) for x in batched_inputs]

    def view_detections(self, views: Sequence[Dict]) -> List[Instances]:
        """the views in view order, in groups of `batch_size`, through model.inference(do_postprocess=False)"""
        out = []
        for lo in range(0, len(views), self.batch_size):
            out.extend(self.model.inference(list(views[lo: lo + self.batch_size]), do_postprocess=False))
        return out

    def _one(self, inp: Dict) -> Dict:
        image = inp["image"]
        height, width = int(inp.get("height", image.shape[1])), int(inp.get("width", image.shape[2]))
        views, tfms = tta_views(self.cfg, image, height, width)
        extra = {k: v for k, v in inp.items() if k not in ("image", "height", "width", "instances")}
        dets = self.view_detections([dict(extra, **v) for v in views])
        return {"instances": merge_detections(dets, tfms, (height, width), self.num_classes, self.nms_thresh, self.topk, self.device)}


def merge_detections(dets: Sequence[Instances], tfms: Sequence[L.BoxTfm], shape_hw: Tuple[int, int], num_classes: int,
                     nms_thresh: float, topk: int, device) -> Instances:
    """one original image: its views' detections (network-input pixels of each view) -> the merged detections"""
    A = len(dets)
    D = max(1, max(len(d) for d in dets))
    boxes = torch.zeros((1, A, D, 4), dtype=torch.float32, device=device)
    scores = torch.zeros((1, A, D), dtype=torch.float32, device=device)
    classes = torch.full((1, A, D), -1, dtype=torch.int32, device=device)
    counts = []
    for a, d in enumerate(dets):
        n = len(d)
        counts.append(n)
        if n:
            boxes[0, a, :n] = d.pred_boxes.tensor.to(device=device, dtype=torch.float32)
            scores[0, a, :n] = d.scores.to(device=device, dtype=torch.float32)
            classes[0, a, :n] = d.pred_classes.to(device=device, dtype=torch.int32)
    count = ops.upload_packed([torch.tensor(counts, dtype=torch.int32)], device)[0].view(1, A)
    ob, os_, oc, on = tta_merge(boxes, scores, classes, count, upload_tfms(tfms, device), num_classes, SCORE_FLOOR, nms_thresh, topk)
    n = int(on.tolist()[0])
    inst = Instances((int(shape_hw[0]), int(shape_hw[1])))
    inst.pred_boxes = Boxes(ob[0, :n])
    inst.scores = os_[0, :n]
    inst.pred_classes = oc[0, :n].to(torch.int64)
    return inst


def tta_merge(boxes, scores, classes, count, tfm, num_classes: int, score_floor: float, nms_thresh: float, topk: int):
    """`aldi_tta_merge` with its workspace and outputs allocated: boxes [B][A][D][4] -> (boxes [B][topk][4], scores, classes, count [B])"""
    B, A, D = int(boxes.shape[0]), int(boxes.shape[1]), int(boxes.shape[2])
    nbytes = ops.tta_merge_workspace(B, A, D)
    if nbytes == 0:
        raise ValueError(f"tta_merge: {A} views x {D} detections exceed the merge's 8192-candidate capacity (or an empty shape)")
    dev = boxes.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ob = torch.empty((B, topk, 4), dtype=torch.float32, device=dev)
    os_ = torch.empty((B, topk), dtype=torch.float32, device=dev)
    oc = torch.empty((B, topk), dtype=torch.int32, device=dev)
    on = torch.empty((B,), dtype=torch.int32, device=dev)
    ops.tta_merge(boxes, scores, classes, count, tfm, num_classes, score_floor, nms_thresh, topk, ws, ob, os_, oc, on)
    return ob, os_, oc, on

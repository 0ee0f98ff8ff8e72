"""Detections back in the original image's coordinates (detectron2 `detector_postprocess`, PARITY UNPINNED).

The geometry runs on the device in float32 (csrc/infer.hip `aldi_detector_postprocess`): every scale is formed here as a Python
double ratio and rounded ONCE to float32 (`box_tfm`), the kernel multiplies, re-orders the corners, clamps and drops the boxes
that became empty.  The tensors stay on the device; the only host read is the per-image count."""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from .structures import Boxes, Instances


def _f32(x) -> float:
    """the one rounding of a double to float32 (as a Python float, exactly representable)"""
    return float(np.float32(x))


def box_tfm(clip_wh: Tuple[float, float], scale0: Tuple[float, float] = (1.0, 1.0), scale1: Tuple[float, float] = (1.0, 1.0),
            flip_w: Optional[float] = None) -> L.BoxTfm:
    """one `aldi_box_tfm`: x -> flip_w - x when `flip_w` is given, then (x, y) *= scale0, then *= scale1, then x clamped to
    [0, clip_wh[0]] and y to [0, clip_wh[1]].  The scales are doubles (ratios formed by the caller); this is the only place
    where they are rounded to float32."""
    t = L.BoxTfm()
    t.flip_w = -1.0 if flip_w is None else _f32(flip_w)
    if flip_w is not None and t.flip_w < 0:
        raise ValueError(f"box_tfm: flip_w {flip_w} is negative")
    t.sx0, t.sy0 = _f32(scale0[0]), _f32(scale0[1])
    t.sx1, t.sy1 = _f32(scale1[0]), _f32(scale1[1])
    t.clip_w, t.clip_h = _f32(clip_wh[0]), _f32(clip_wh[1])
    t.pad = 0
    return t


def upload_tfms(tfms: Sequence[L.BoxTfm], device) -> torch.Tensor:
    """descriptors -> device bytes, through one pinned staging buffer"""
    n = len(tfms)
    arr = (L.BoxTfm * max(n, 1))(*tfms)
    host = torch.empty(ctypes.sizeof(arr), dtype=torch.uint8).pin_memory()
    ctypes.memmove(host.data_ptr(), ctypes.addressof(arr), ctypes.sizeof(arr))
    return host.to(device, non_blocking=True)


def postprocess_batch(boxes: torch.Tensor, scores: torch.Tensor, classes: torch.Tensor, count: torch.Tensor,
                      image_sizes: Sequence[Tuple[int, int]], output_sizes: Sequence[Tuple[int, int]]) -> List[Instances]:
    """boxes [N][D][4] float32, scores [N][D], classes [N][D] int32, count [N] int32 (device tensors in network-input pixels of
    `image_sizes` (h, w)) -> one Instances per image in the pixels of `output_sizes` (height, width)"""
    N, D = int(boxes.shape[0]), int(boxes.shape[1])
    if not (len(image_sizes) == N and len(output_sizes) == N):
        raise ValueError("postprocess_batch: one image size and one output size per image")
    if N == 0:
        return []
    if D == 0:                                                   # (nothing to transform, and an empty tensor has no address to pass)
        return [Instances((int(oh), int(ow)), pred_boxes=Boxes(boxes[i].reshape(0, 4).float()), scores=scores[i].reshape(0).float(),
                          pred_classes=classes[i].reshape(0).to(torch.int64)) for i, (oh, ow) in enumerate(output_sizes)]
    boxes, scores = boxes.contiguous().float(), scores.contiguous().float()
    classes, count = classes.contiguous().to(torch.int32), count.contiguous().to(torch.int32)
    tf = upload_tfms([box_tfm((ow, oh), (ow / iw, oh / ih)) for (ih, iw), (oh, ow) in zip(image_sizes, output_sizes)], boxes.device)
    ob, os_, oc = torch.empty_like(boxes), torch.empty_like(scores), torch.empty_like(classes)
    on = torch.empty_like(count)
    ops.detector_postprocess(boxes, scores, classes, count, tf, ob, os_, oc, on)
    out = []
    for i, n in enumerate(on.tolist()):
        inst = Instances((int(output_sizes[i][0]), int(output_sizes[i][1])))
        inst.pred_boxes = Boxes(ob[i, :n])
        inst.scores = os_[i, :n]
        inst.pred_classes = oc[i, :n].to(torch.int64)
        out.append(inst)
    return out


def output_sizes(batched_inputs: Sequence[dict], image_sizes: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """detectron2 `GeneralizedRCNN._postprocess`: input.get("height", image_size[0]), input.get("width", image_size[1])"""
    return [(int(inp.get("height", sz[0])), int(inp.get("width", sz[1]))) for inp, sz in zip(batched_inputs, image_sizes)]


def detector_postprocess(results, output_height, output_width):
    """detectron2 `detector_postprocess` for boxes: `results` is one `Instances` in network-input pixels (pred_boxes, scores,
    pred_classes on the device) -> a new `Instances` with image_size = (output_height, output_width); or an engine's inference
    context (`det` with boxes [N][D][4] / scores / classes / count, and `sizes`) with one height and one width per image -> a
    list of them.  Scales are output_width / image_size[1] and output_height / image_size[0]."""
    if isinstance(results, Instances):
        b = results.pred_boxes.tensor.reshape(1, -1, 4)
        n = int(b.shape[1])
        dev = b.device
        if dev.type != "cuda":
            raise TypeError("detector_postprocess runs on the device: move the Instances there first")
        cnt = torch.full((1,), n, dtype=torch.int32, device=dev)
        return postprocess_batch(b, results.scores.reshape(1, n), results.pred_classes.reshape(1, n), cnt, [tuple(results.image_size)],
                                 [(int(output_height), int(output_width))])[0]
    d = results.det
    hs = [output_height] * len(results.sizes) if np.isscalar(output_height) else list(output_height)
    ws = [output_width] * len(results.sizes) if np.isscalar(output_width) else list(output_width)
    return postprocess_batch(d.boxes, d.scores, d.classes, d.count, list(results.sizes), list(zip(hs, ws)))

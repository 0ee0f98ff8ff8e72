"""CPU restatements for the inference API tests (tests/test_infer_cpu.py, tests/test_infer_gpu.py).  They share no code with
aldi_amd: detectron2 v0.6's detector_postprocess / TransformList.inverse().apply_box / _merge_detections restated on float32
arrays, one operation per stage, in the order the device kernels state in include/aldi_hip.h.

A descriptor here is a plain dict of numpy float32 scalars: flip_w (< 0: no flip), sx0, sy0, sx1, sy1, clip_w, clip_h."""
import numpy as np
import torch


def desc(clip_wh, scale0=(1.0, 1.0), scale1=(1.0, 1.0), flip_w=None):
    """scales are Python doubles (ratios); each is rounded once to float32"""
    f = np.float32
    return dict(flip_w=f(-1.0) if flip_w is None else f(flip_w), sx0=f(scale0[0]), sy0=f(scale0[1]), sx1=f(scale1[0]), sy1=f(scale1[1]),
                clip_w=f(clip_wh[0]), clip_h=f(clip_wh[1]))


def view_desc(h, w, new_h, new_w, flip, height, width):
    """a test-time view (h, w) -> (new_h, new_w), flipped or not, of an input image that is itself a resize of the (height, width)
    original: un-flip, view -> input image, input image -> original, clip"""
    return desc((width, height), (w / new_w, h / new_h), (width / w, height / h), new_w if flip else None)


def tfm_numpy(boxes, d):
    """[n, 4] float32 XYXY through one descriptor, numpy float32 throughout"""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4).copy()
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        if d["flip_w"] >= 0:
            x1, x2 = d["flip_w"] - x1, d["flip_w"] - x2
        x1, y1, x2, y2 = x1 * d["sx0"], y1 * d["sy0"], x2 * d["sx0"], y2 * d["sy0"]
        x1, y1, x2, y2 = x1 * d["sx1"], y1 * d["sy1"], x2 * d["sx1"], y2 * d["sy1"]
        lo_x, hi_x, lo_y, hi_y = np.minimum(x1, x2), np.maximum(x1, x2), np.minimum(y1, y2), np.maximum(y1, y2)
        zero = np.float32(0)
        out = np.stack([np.clip(lo_x, zero, d["clip_w"]), np.clip(lo_y, zero, d["clip_h"]),
                        np.clip(hi_x, zero, d["clip_w"]), np.clip(hi_y, zero, d["clip_h"])], axis=1)
    assert out.dtype == np.float32
    return out


def postprocess(boxes, scores, classes, count, descs):
    """boxes [N][D][4] float32, scores [N][D] float32, classes [N][D] int32, count [N] (CPU torch tensors) -> the same shapes
    + count [N] int32; torch float32 tensor operations; rows from the count on are zero boxes, zero scores, class -1"""
    N, D = boxes.shape[:2]
    ob, os_, oc = torch.zeros(N, D, 4, dtype=torch.float32), torch.zeros(N, D, dtype=torch.float32), torch.full((N, D), -1, dtype=torch.int32)
    on = torch.zeros(N, dtype=torch.int32)
    for n in range(N):
        c = min(max(int(count[n]), 0), D)
        d = descs[n]
        b = boxes[n, :c].clone().to(torch.float32)
        x1, y1, x2, y2 = b.unbind(1)
        if float(d["flip_w"]) >= 0:
            fw = torch.tensor(float(d["flip_w"]), dtype=torch.float32)
            x1, x2 = fw - x1, fw - x2
        for sx, sy in ((d["sx0"], d["sy0"]), (d["sx1"], d["sy1"])):
            sx, sy = torch.tensor(float(sx), dtype=torch.float32), torch.tensor(float(sy), dtype=torch.float32)
            x1, y1, x2, y2 = x1 * sx, y1 * sy, x2 * sx, y2 * sy
        lx, hx, ly, hy = torch.minimum(x1, x2), torch.maximum(x1, x2), torch.minimum(y1, y2), torch.maximum(y1, y2)
        lx, hx = lx.clamp(min=0, max=float(d["clip_w"])), hx.clamp(min=0, max=float(d["clip_w"]))
        ly, hy = ly.clamp(min=0, max=float(d["clip_h"])), hy.clamp(min=0, max=float(d["clip_h"]))
        assert lx.dtype == torch.float32
        keep = ((hx - lx) > 0) & ((hy - ly) > 0)
        k = int(keep.sum())
        ob[n, :k] = torch.stack([lx, ly, hx, hy], 1)[keep]
        os_[n, :k] = scores[n, :c][keep]
        oc[n, :k] = classes[n, :c][keep].to(torch.int32)
        on[n] = k
    return ob, os_, oc, on


def merge(boxes, scores, classes, count, descs, K, score_floor, nms_thresh, topk):
    """one original image: boxes [A][D][4], scores / classes [A][D], count [A] (numpy), descs [A] -> (boxes [topk][4] float32,
    scores [topk] float32, classes [topk] int32, count): the inverse transform in numpy float32, then
    oracle.d2_rcnn.batched_nms (per class, IoU > thresh suppresses, stable descending score order) and a [:topk] cut"""
    from oracle import d2_rcnn as d2
    boxes, scores, classes = np.asarray(boxes, np.float32), np.asarray(scores, np.float32), np.asarray(classes, np.int32)
    A, D = scores.shape
    cb, cs, cc = [], [], []
    for a in range(A):                                     # candidates in flat-index order a * D + j
        c = min(max(int(count[a]), 0), D)
        if c == 0:
            continue
        b, s, k = boxes[a, :c], scores[a, :c], classes[a, :c]
        ok = np.isfinite(b).all(axis=1) & np.isfinite(s) & (k >= 0) & (k < K)
        t = tfm_numpy(b[ok], descs[a])
        s, k = s[ok], k[ok]
        above = s > np.float32(score_floor)
        cb.append(t[above]); cs.append(s[above]); cc.append(k[above])
    ob, os_, oc = np.zeros((topk, 4), np.float32), np.zeros(topk, np.float32), np.full(topk, -1, np.int32)
    if not cb or sum(len(x) for x in cs) == 0:
        return ob, os_, oc, 0
    cb, cs, cc = np.concatenate(cb), np.concatenate(cs), np.concatenate(cc)
    keep = d2.batched_nms(torch.from_numpy(cb), torch.from_numpy(cs), torch.from_numpy(cc.astype(np.int64)), float(np.float32(nms_thresh)))
    keep = keep[:topk].numpy()
    n = len(keep)
    ob[:n], os_[:n], oc[:n] = cb[keep], cs[keep], cc[keep]
    return ob, os_, oc, n


def directed_merge_case():
    """(boxes [3][6][4], scores, classes, count, expected rows): every rule of aldi_tta_merge once, identity transforms"""
    nan, inf = float("nan"), float("inf")
    v0 = [([0, 0, 2, 2], 0.9, 0), ([0, 0, 2, 1], 0.8, 0),                  # IoU exactly 0.5 at threshold 0.5: both survive (strict)
          ([10, 10, 20, 20], 0.7, 1), ([10, 10, 20, 20], 0.6, 2),          # the same box, two classes: both survive
          ([30, 30, 40, 40], 0.5, 0),                                      # ties view 1's row 0: the lower flat index first
          ([10, 10, 20, 20], 0.65, 1)]                                     # suppressed by the 0.7 box of its class
    v1 = [([50, 50, 60, 60], 0.5, 0),
          ([70, 70, 80, 80], float(np.float32(1e-8)), 0),                           # score == the floor: dropped (strict)
          ([nan, 0, 5, 5], 0.95, 0), ([0, 50, 5, 55], inf, 0),             # NaN coordinate, Inf score: dropped
          ([0, 60, 5, 65], 0.99, 3), ([0, 70, 5, 75], 0.97, -1)]           # class == K, class < 0: dropped
    v2 = [([5, 80, 25, 95], 0.999, 1)] * 6                                 # a view with count 0: its rows are never read
    views = (v0, v1, v2)
    boxes = np.array([[r[0] for r in v] for v in views], dtype=np.float32)
    scores = np.array([[r[1] for r in v] for v in views], dtype=np.float32)
    classes = np.array([[r[2] for r in v] for v in views], dtype=np.int32)
    expected = [v0[0], v0[1], v0[2], v0[3], v0[4], v1[0]]
    return boxes, scores, classes, np.array([6, 6, 0], np.int32), expected

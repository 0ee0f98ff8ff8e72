"""Pillow's `Image.resize(size, BILINEAR)` for uint8 images restated in numpy: the reference of the weak-view tests.

Written from Pillow's ImagingResample (precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
Vertical_8bpc) and sharing no code with aldi_amd: scalar loops in the C source's order, one output index at a time.
tests/golden/pil_bilinear.npz holds Pillow's own bytes; tests/test_weak_aug_cpu.py holds this file to them."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _triangle(a: float) -> float:
    a = -a if a < 0.0 else a
    return 1.0 - a if a < 1.0 else 0.0


def coefficients(insz: int, outsz: int):
    """-> (ksize, bounds [(xmin, n)] * outsz, kk [[int] * ksize] * outsz)"""
    scale = insz / outsz
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, kk = [], []
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > insz:
            xmax = insz
        n = xmax - xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(n):
            w = _triangle((x + xmin - center + 0.5) * ss)
            k[x] = w
            ww += w
        for x in range(n):
            if ww != 0.0:
                k[x] /= ww
        bounds.append((xmin, n))
        kk.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
    return ksize, bounds, kk


def _pass(img: np.ndarray, outsz: int, axis: int) -> np.ndarray:
    """one pass along `axis` (0 rows / 1 columns) of an (H, W, C) uint8 image, result rounded to uint8"""
    insz = img.shape[axis]
    _, bounds, kk = coefficients(insz, outsz)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((outsz,) + src.shape[1:], dtype=np.uint8)
    for xx in range(outsz):
        xmin, n = bounds[xx]
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(n):
            acc += src[xmin + x] * kk[xx][x]
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """(H, W, C) uint8 -> (new_h, new_w, C) uint8: horizontal pass first (only if the width changes), then vertical"""
    assert img.dtype == np.uint8 and img.ndim == 3
    out = img
    if new_w != img.shape[1]:
        out = _pass(out, new_w, 1)
    if new_h != img.shape[0]:
        out = _pass(out, new_h, 0)
    return out.copy() if out is img else out


def weak_view(img: np.ndarray, new_h: int, new_w: int, flip: bool) -> np.ndarray:
    """resize, then detectron2's HFlipTransform (np.flip along the width)"""
    out = resize(img, new_h, new_w)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out

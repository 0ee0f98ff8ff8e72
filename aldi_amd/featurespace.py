"""Feature-space PCA of a source and a target test set, image- and proposal-level: the domain-gap picture of the reference's
tools/visualize_featurespace.py, with the pooling, the moments and the projection on the device.

The reference hooks the backbone and the box pooler, copies every pooled map to the host and fits scikit-learn's PCA on the
concatenated rows.  Here `RCNN.feature_pass` pools on the device (csrc/featstat.hip), `aldi_moments_accum` keeps the fp64 first and
second moments of both levels in HBM, the host receives one (1 + C + C * C)-word block per level, diagonalises the covariance
(torch.linalg.eigh on the CPU, 256 x 256) and `aldi_project2` maps the kept rows onto the top two components.

Memory: a kept row is C = 256 fp32 values = 1 KB on the device.  The image level keeps one row per image; the proposal level one per
real proposal (up to RPN.POST_NMS_TOPK_TEST = 1000 per image, i.e. about 1 MB per image).  `keep_features=False` keeps the moments
only (513 KB per level, independent of the data set's size) and yields no coordinates.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

LEVELS = ("image", "proposal")


class FeatureSpaceError(ValueError):
    """the accumulated statistics do not define a PCA (fewer than two rows) or a request names an unknown level"""


def select_datasets(train: Sequence[str], test: Sequence[str]) -> Tuple[str, str]:
    """(source, target) as the reference's tool picks them: two DATASETS.TEST names, or one DATASETS.TRAIN name plus one
    DATASETS.TEST name; anything else is ambiguous"""
    train, test = list(train), list(test)
    if len(test) == 2:
        return test[0], test[1]
    if len(test) == 1 and len(train) == 1:
        return train[0], test[0]
    raise ValueError(f"Ambiguous which datasets represent source and target (DATASETS.TRAIN {tuple(train)}, DATASETS.TEST {tuple(test)}): "
                     "name two test sets, or one training and one test set")


def moments_to_mean_cov(sum_, gram, count) -> Tuple[np.ndarray, np.ndarray, int]:
    """(sum [C], gram = X^T X [C][C], count n) -> (mean, unbiased covariance (G - n mu mu^T) / (n - 1), n), fp64"""
    s = np.asarray(sum_, dtype=np.float64).reshape(-1)
    g = np.asarray(gram, dtype=np.float64)
    n = int(round(float(count)))
    if g.shape != (s.size, s.size):
        raise FeatureSpaceError(f"gram matrix of shape {g.shape} does not match a sum of {s.size} entries")
    if n < 2:
        raise FeatureSpaceError(f"a PCA needs at least two feature rows, the accumulators hold {n}")
    mean = s / n
    cov = (g - n * np.outer(mean, mean)) / (n - 1)
    return mean, 0.5 * (cov + cov.T), n


def pca_from_moments(sum_, gram, count, k: int = 2) -> Dict[str, np.ndarray]:
    """The top-k principal components from accumulated moments: components [k][C] (unit rows, descending variance),
    explained_variance [k], explained_variance_ratio [k] (of the total variance), mean [C], count.
    Sign: the largest-magnitude loading of every component is positive -- scikit-learn >= 1.5's
    svd_flip(u_based_decision=False), a function of the component alone, so independent of the order the rows arrived in."""
    mean, cov, n = moments_to_mean_cov(sum_, gram, count)
    w, v = torch.linalg.eigh(torch.from_numpy(cov))                       # ascending eigenvalues, CPU, fp64
    w, v = w.numpy()[::-1], v.numpy()[:, ::-1]
    comp = np.ascontiguousarray(v[:, :k].T)
    top = np.abs(comp).argmax(axis=1)
    comp *= np.sign(comp[np.arange(comp.shape[0]), top])[:, None]
    total = float(np.trace(cov))
    ev = np.maximum(w[:k], 0.0)
    return {"components": comp, "explained_variance": ev, "explained_variance_ratio": ev / total if total > 0 else np.zeros_like(ev),
            "mean": mean, "count": n}


class _Accumulator:
    """fp64 device block [count, sum (C), gram (C x C)] of one level: one copy brings it to the host"""

    def __init__(self, C: int, device):
        self.C = C
        self.block = torch.zeros(1 + C + C * C, dtype=torch.float64, device=device)
        self.count, self.sum, self.gram = self.block[:1], self.block[1:1 + C], self.block[1 + C:].view(C, C)

    def host(self):
        b = self.block.cpu().numpy()
        return b[1:1 + self.C], b[1 + self.C:].reshape(self.C, self.C), b[0]


class FeatureSpaceCollector:
    """collect(name, loader) for every data set, then pca("image") / pca("proposal").

    One set of moment accumulators per level is shared by all data sets (the PCA is fitted on their union, as the reference's);
    with `keep_features` the pooled rows stay on the device (1 KB per row: see the module docstring) and `pca` also returns their
    coordinates per data set.  Single process only."""

    def __init__(self, model, pooling: str = "avg", keep_features: bool = True):
        from . import ops
        from .arch import FPN_C
        from .engine import RCNN
        engine = getattr(model, "engine", None)
        if type(engine) is not RCNN:
            raise ValueError("FeatureSpaceCollector: only the R50-FPN engine is supported (feature-space PCA is not wired for the ViTDet, "
                             f"ConvNeXt or Deformable-DETR engines); this model runs on {type(engine).__name__}")
        ops._pool_mode(pooling)
        self.model, self.engine, self.pooling, self.keep_features = model, engine, pooling, keep_features
        dev = engine.device
        self._ops = ops
        self._acc = {lvl: _Accumulator(FPN_C, dev) for lvl in LEVELS}
        self._ws = ops.moments_workspace(FPN_C, dev)
        self._chunks: Dict[str, Dict[str, list]] = {}
        self._counts: Dict[str, Dict[str, torch.Tensor]] = {}

    @property
    def names(self):
        return list(self._counts)

    def collect(self, name: str, data_loader) -> None:
        """run `feature_pass` over the loader's batches (lists of {"image": uint8 CHW}; `ALDITrainer.build_test_loader`'s
        (batches, records) pair is accepted as is) and accumulate both levels"""
        ops = self._ops
        if isinstance(data_loader, tuple):
            data_loader = data_loader[0]
        dev = self.engine.device
        counts = self._counts.setdefault(name, {lvl: torch.zeros(1, dtype=torch.int64, device=dev) for lvl in LEVELS})
        chunks = self._chunks.setdefault(name, {lvl: [] for lvl in LEVELS})
        with torch.no_grad():
            for batch in data_loader:
                img, prop, total = self.engine.feature_pass([b["image"] for b in batch], self.pooling)
                a = self._acc["image"]
                ops.moments_accum(img, a.sum, a.gram, a.count, self._ws)
                a = self._acc["proposal"]
                ops.moments_accum(prop, a.sum, a.gram, a.count, self._ws, n_dev=total)
                counts["image"] += img.shape[0]
                counts["proposal"] += total
                if self.keep_features:
                    chunks["image"].append(img)
                    k = int(total)                      # (the one host wait of a kept pass: the rows to keep)
                    if k:
                        chunks["proposal"].append(prop[:k].clone())

    def count(self, name: str, level: str) -> int:
        self._check_level(level)
        return int(self._counts[name][level])

    def features(self, name: str, level: str) -> torch.Tensor:
        """the kept rows of one data set (device, fp32 [n][C])"""
        self._check_level(level)
        if not self.keep_features:
            raise FeatureSpaceError("features were not kept (keep_features=False)")
        ch = self._chunks[name][level]
        C = self._acc[level].C
        return torch.cat(ch) if ch else torch.zeros((0, C), dtype=torch.float32, device=self.engine.device)

    def _check_level(self, level: str):
        if level not in LEVELS:
            raise FeatureSpaceError(f"level must be one of {LEVELS}, got {level!r}")

    def moments(self, level: str) -> Dict[str, np.ndarray]:
        """mean [C], covariance [C][C] (unbiased) and count of the union of everything collected, plus the raw fp64 sum / gram"""
        self._check_level(level)
        s, g, n = self._acc[level].host()
        mean, cov, n = moments_to_mean_cov(s, g, n)
        return {"mean": mean, "cov": cov, "count": n, "sum": s.copy(), "gram": g.copy()}

    def pca(self, level: str) -> Dict[str, object]:
        """components (2, C), mean (C,), explained_variance_ratio (2,), count -- and, when the features were kept,
        coords {name: (n, 2) fp32} (aldi_project2 on the device, copied to the host)"""
        self._check_level(level)
        res: Dict[str, object] = pca_from_moments(*self._acc[level].host())
        if self.keep_features:
            ops, dev = self._ops, self.engine.device
            mean = torch.from_numpy(np.ascontiguousarray(res["mean"])).to(dev)
            comp = torch.from_numpy(np.ascontiguousarray(res["components"])).to(dev)
            coords = {}
            for name in self._counts:
                parts = [ops.project2(x, mean, comp) for x in self._chunks[name][level]]
                coords[name] = (torch.cat(parts) if parts else torch.zeros((0, 2), dtype=torch.float32, device=dev)).cpu().numpy()
            res["coords"] = coords
        return res

"""`Predictor`: detectron2's `DefaultPredictor` on the device -- a raw image in, `{"instances": Instances}` in that image's
coordinates out.  The test-time resize is the Pillow-exact device resize of `aug.weak_views`."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import aug


class Predictor:
    """Builds the model of `cfg`, loads `cfg.MODEL.WEIGHTS` when it is not empty, and puts the model in eval mode.

    The weights go through the project's checkpointer: with `EMA.LOAD_FROM_EMA_ON_START` it is `DetectionCheckpointerWithEMA`,
    which starts from the checkpoint's "ema" weights when the file has them (the reference's `--eval-only` branch,
    tools/train_net.py:67-76); without it the plain `DetectionCheckpointer` loads the "model" entry."""

    def __init__(self, cfg, model=None):
        from .checkpoint import DetectionCheckpointer, DetectionCheckpointerWithEMA
        from .model import build_aldi
        self.cfg = cfg
        self.model = build_aldi(cfg) if model is None else model
        if model is None and cfg.MODEL.WEIGHTS:
            ckpt_cls = DetectionCheckpointerWithEMA if cfg.EMA.LOAD_FROM_EMA_ON_START else DetectionCheckpointer
            ckpt_cls(self.model, save_dir=cfg.OUTPUT_DIR).resume_or_load(cfg.MODEL.WEIGHTS, resume=False)
        self.model.eval()
        self.device = torch.device(cfg.MODEL.DEVICE)
        self.input_format = cfg.INPUT.FORMAT
        if self.input_format not in ("RGB", "BGR"):
            raise ValueError(f"Predictor: INPUT.FORMAT {self.input_format!r} is neither 'RGB' nor 'BGR'")
        # built directly: get_weak_augs refuses configs with INPUT.CROP.ENABLED even at test time, where no crop is applied
        self.min_size, self.max_size = int(cfg.INPUT.MIN_SIZE_TEST), int(cfg.INPUT.MAX_SIZE_TEST)
        self.aug = aug.ResizeShortestEdge((self.min_size, self.min_size), self.max_size, "choice")

    def _device_image(self, image) -> torch.Tensor:
        """uint8 (H, W, 3), numpy or tensor, host or device, BGR as cv2.imread gives it -> contiguous device tensor in the
        model's channel order"""
        t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else image
        if not (torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3):
            raise ValueError("Predictor: the image must be uint8 of shape (H, W, 3)")
        t = t.to(self.device)
        if self.input_format == "RGB":
            t = t.flip(2)
        return t.contiguous()

    def views(self, images: Sequence) -> List[Dict]:
        """the model's inputs for raw images: ResizeShortestEdge(MIN_SIZE_TEST, MAX_SIZE_TEST) (MIN_SIZE_TEST 0: the size is
        kept), no flip, nothing drawn; "height" / "width" are the raw image's"""
        dev = [self._device_image(im) for im in images]
        params = []
        for t in dev:
            h, w = int(t.shape[0]), int(t.shape[1])
            nh, nw = (h, w) if self.min_size == 0 else self.aug.get_output_shape(h, w, self.min_size, self.max_size)
            params.append(aug.WeakParams(h, w, nh, nw, False))
        outs = aug.weak_views(dev, params, chw_out=True, chw_in=False)
        return [{"image": o, "height": p.h, "width": p.w} for o, p in zip(outs, params)]

    def batch(self, images: Sequence) -> List[Dict]:
        """a (ragged) list of raw images -> one result per image: one resize call, one inference call"""
        if len(images) == 0:
            return []
        with torch.no_grad():
            return self.model.inference(self.views(images), do_postprocess=True)

    def __call__(self, image) -> Dict:
        return self.batch([image])[0]

"""Reading images and the dataset mapper: the host half of a file-backed loader.  PARITY UNPINNED restatements of
detectron2 v0.6 `data/detection_utils.py` (`read_image`, `check_image_size`, `annotations_to_instances`) and `data/dataset_mapper.py`,
boxes only.

Everything here is host work that a decode thread may run: it reads, decodes and builds numpy arrays and CPU tensors.  It makes no
device call of any kind -- no pinning, no copy, no launch -- and applies NO geometry and NO channel exchange: the device view
(aldi_amd/aug.py `launch_views`) crops, resizes, flips and exchanges R and B from the drawn `ViewParams`, and the loader stage
transforms the instances from the same parameters."""
from __future__ import annotations

import os
from typing import Tuple

import numpy as np
import torch

from .datasets import XYWH_ABS

NO_PILLOW_FORMATS = ".npy (uint8 H x W x 3) and binary .ppm (P6, maxval 255)"
_EXIF_ORIENTATION = 0x0112


def _swap_for(format: str) -> bool:
    if format not in ("RGB", "BGR"):
        raise ValueError(f"read_image: format {format!r} is neither 'RGB' nor 'BGR'")
    return format == "BGR"


def _read_npy(file_name: str) -> np.ndarray:
    try:
        img = np.load(file_name, allow_pickle=False)
    except (ValueError, EOFError, OSError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise ValueError(f"{file_name}: not a readable .npy file ({e})") from e
    if not (isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] > 0 and img.shape[1] > 0):
        raise ValueError(f"{file_name}: expected a uint8 array of shape (H, W, 3), got {getattr(img, 'dtype', None)} {getattr(img, 'shape', None)}")
    return np.ascontiguousarray(img)


def _read_ppm(file_name: str) -> np.ndarray:
    """binary PPM: "P6" width height maxval, separated by whitespace with `#` comments to the end of a line, ONE whitespace byte, then
    height * width * 3 bytes"""
    with open(file_name, "rb") as f:
        head = f.read(4096)
    pos, tokens = 0, []
    while len(tokens) < 4 and pos < len(head):
        c = head[pos: pos + 1]
        if c.isspace():
            pos += 1
        elif c == b"#":
            nl = head.find(b"\n", pos)
            pos = len(head) if nl < 0 else nl + 1
        else:
            end = pos
            while end < len(head) and not head[end: end + 1].isspace() and head[end: end + 1] != b"#":
                end += 1
            tokens.append(head[pos:end])
            pos = end
    if len(tokens) < 4 or tokens[0] != b"P6" or not all(t.isdigit() for t in tokens[1:]) or pos >= len(head) or not head[pos: pos + 1].isspace():
        raise ValueError(f"{file_name}: not a binary PPM (P6) file, or its header is truncated")
    w, h, maxval = (int(t) for t in tokens[1:])
    if maxval != 255 or w < 1 or h < 1:
        raise ValueError(f"{file_name}: PPM of {w}x{h} with maxval {maxval}: only non-empty 8-bit images (maxval 255) are read")
    offset, need, have = pos + 1, h * w * 3, os.path.getsize(file_name)
    if have - offset != need:
        raise ValueError(f"{file_name}: PPM header says {w}x{h} ({need} bytes of pixels), the file holds {max(have - offset, 0)}: "
                         f"{'truncated' if have - offset < need else 'mis-sized'}")
    img = np.fromfile(file_name, dtype=np.uint8, count=need, offset=offset)
    if img.size != need:
        raise ValueError(f"{file_name}: truncated PPM: {img.size} of {need} bytes of pixels")
    return img.reshape(h, w, 3)


def _read_pillow(file_name: str) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError:
        raise ImportError(f"{file_name}: reading this format needs Pillow, which is not installed; {NO_PILLOW_FORMATS} are read without it") from None
    try:
        with Image.open(file_name) as im:
            # detectron2 `_apply_exif_orientation`: the tag says how the stored pixels are to be turned
            method = {2: Image.FLIP_LEFT_RIGHT, 3: Image.ROTATE_180, 4: Image.FLIP_TOP_BOTTOM, 5: Image.TRANSPOSE, 6: Image.ROTATE_270,
                      7: Image.TRANSVERSE, 8: Image.ROTATE_90}.get(im.getexif().get(_EXIF_ORIENTATION))
            if method is not None:
                im = im.transpose(method)
            img = np.array(im.convert("RGB"))                          # (a copy: writable, as torch.from_numpy wants it)
    except FileNotFoundError:
        raise
    except Exception as e:                                             # (Pillow raises OSError, SyntaxError, ValueError, ... for bad files)
        raise ValueError(f"{file_name}: cannot be decoded ({type(e).__name__}: {e})") from e
    return np.ascontiguousarray(img, dtype=np.uint8)


def read_image(file_name: str, format: str = "BGR") -> Tuple[np.ndarray, bool]:
    """-> (uint8 (H, W, 3) array in RGB order, swap_rb).  `swap_rb` says that `format` ("BGR") wants channels 0 and 2 exchanged; the
    exchange itself is the device view's SWAP_RB, never done here.  `.npy` and binary `.ppm` are parsed with numpy alone; every
    other extension goes through Pillow (`Image.open(f).convert("RGB")` with the EXIF orientation applied, as detectron2 does), and
    raises an ImportError that names the file where Pillow is missing.  A truncated or mis-sized file raises a ValueError that names it."""
    swap = _swap_for(format)
    ext = os.path.splitext(file_name)[1].lower()
    if ext == ".npy":
        return _read_npy(file_name), swap
    if ext == ".ppm":
        return _read_ppm(file_name), swap
    return _read_pillow(file_name), swap


def check_image_size(dataset_dict: dict, image: np.ndarray) -> None:
    """detectron2's: the record's `width` / `height`, when present, must be the decoded size; absent ones are filled in"""
    h, w = int(image.shape[0]), int(image.shape[1])
    if "width" in dataset_dict or "height" in dataset_dict:
        expected = (dataset_dict.get("height", h), dataset_dict.get("width", w))
        if expected != (h, w):
            raise ValueError(f"Mismatched image shape for image {dataset_dict.get('file_name', '')}: the decoded image is "
                             f"{h}x{w} (height x width), the dataset record says {expected[0]}x{expected[1]}")
    dataset_dict.setdefault("width", w)
    dataset_dict.setdefault("height", h)


class DatasetMapper:
    """dataset dict -> {image_raw: host uint8 (H, W, 3) tensor in RGB order (neither pinned nor on the device), file_name, image_id,
    height, width, instances: {image_size, gt_boxes float32 XYXY, gt_classes int64}}.  Crowd annotations are dropped when training
    (detectron2's mapper); `labeled=False` is the reference's UnlabeledDatasetMapper: empty boxes and classes.  `swap_rb` is what the
    device view has to be told for INPUT.FORMAT."""

    def __init__(self, cfg, is_train: bool = True, labeled: bool = True):
        self.format = str(cfg.INPUT.FORMAT)
        self.swap_rb = _swap_for(self.format)
        self.is_train, self.labeled = bool(is_train), bool(labeled)

    def __call__(self, dataset_dict: dict) -> dict:
        d = dict(dataset_dict)                                         # (the catalog's record is shared: never modified)
        img, _ = read_image(d["file_name"], self.format)
        check_image_size(d, img)
        h, w = int(img.shape[0]), int(img.shape[1])
        annos = [a for a in d.get("annotations", []) if not (self.is_train and a.get("iscrowd", 0) != 0)] if self.labeled else []
        boxes = np.zeros((len(annos), 4), dtype=np.float64)
        for i, a in enumerate(annos):
            if a.get("bbox_mode", XYWH_ABS) != XYWH_ABS:
                raise ValueError(f"{d['file_name']}: annotation with bbox_mode {a.get('bbox_mode')!r}; the COCO records carry {XYWH_ABS}")
            x, y, bw, bh = (float(v) for v in a["bbox"])
            boxes[i] = (x, y, x + bw, y + bh)
        inst = {"image_size": (h, w), "gt_boxes": torch.from_numpy(boxes.astype(np.float32)),
                "gt_classes": torch.tensor([int(a["category_id"]) for a in annos], dtype=torch.int64)}
        return {"image_raw": torch.from_numpy(img), "file_name": d["file_name"], "image_id": d.get("image_id"), "height": h, "width": w,
                "instances": inst}

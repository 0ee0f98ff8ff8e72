"""Datasets on disk: detectron2's catalogs and COCO-json reader restated with the `json` module (reference
aldi/datasets.py registers its datasets through detectron2's `register_coco_instances`).  PARITY UNPINNED restatements of
detectron2 v0.6 `data/catalog.py`, `data/datasets/coco.py` (`load_coco_json`) and `data/build.py`
(`get_detection_dataset_dicts`), boxes only.  Nothing is registered at import: the catalog starts empty."""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional, Sequence

XYWH_ABS = "XYWH_ABS"


class _DatasetCatalog:
    """name -> a function that returns the list of records (called each time: `register_coco_instances` caches its own)"""
    def __init__(self):
        self._fns: Dict[str, Callable[[], List[dict]]] = {}

    def register(self, name: str, func: Callable[[], List[dict]]) -> None:
        if not callable(func):
            raise TypeError("DatasetCatalog.register: the second argument must be a function that returns the records")
        if name in self._fns:
            raise ValueError(f"Dataset '{name}' is already registered!")
        self._fns[name] = func

    def get(self, name: str) -> List[dict]:
        if name not in self._fns:
            raise KeyError(f"Dataset '{name}' is not registered! Available datasets are: {', '.join(self.list())}")
        return self._fns[name]()

    def list(self) -> List[str]:
        return list(self._fns)

    def remove(self, name: str) -> None:
        self._fns.pop(name)

    def __contains__(self, name: str) -> bool:
        return name in self._fns


class _MetadataCatalog:
    """name -> a namespace of metadata (`thing_classes`, `thing_dataset_id_to_contiguous_id`, `json_file`, `image_root`, ...),
    created empty on first `get`, as detectron2's"""
    def __init__(self):
        self._meta: Dict[str, SimpleNamespace] = {}

    def get(self, name: str) -> SimpleNamespace:
        if name not in self._meta:
            self._meta[name] = SimpleNamespace(name=name)
        return self._meta[name]

    def list(self) -> List[str]:
        return list(self._meta)

    def remove(self, name: str) -> None:
        self._meta.pop(name)

    def __contains__(self, name: str) -> bool:
        return name in self._meta


DatasetCatalog = _DatasetCatalog()
MetadataCatalog = _MetadataCatalog()


def load_coco_json(json_file: str, image_root: str, dataset_name: Optional[str] = None) -> List[dict]:
    """COCO instances json -> detectron2-format records, images in ascending id order: file_name = join(image_root, file_name),
    height, width, image_id, annotations = [bbox (XYWH_ABS), bbox_mode, iscrowd, area, category_id mapped to 0..K-1 by ascending
    category id].  With `dataset_name` the metadata gets `thing_classes` (the category names in id order) and
    `thing_dataset_id_to_contiguous_id`.  Every error names the file and the offending id."""
    with open(json_file) as f:
        data = json.load(f)
    cats = sorted(data.get("categories", []), key=lambda c: c["id"])
    cat_ids = [c["id"] for c in cats]
    if len(set(cat_ids)) != len(cat_ids):
        raise ValueError(f"{json_file}: category ids are not unique: {cat_ids}")
    id_map = {cid: i for i, cid in enumerate(cat_ids)}
    if dataset_name is not None:
        meta = MetadataCatalog.get(dataset_name)
        meta.thing_classes = [c["name"] for c in cats]
        meta.thing_dataset_id_to_contiguous_id = id_map
    images = sorted(data.get("images", []), key=lambda im: im["id"])
    if len({im["id"] for im in images}) != len(images):
        raise ValueError(f"{json_file}: image ids are not unique")
    per_image: Dict[object, List[dict]] = {im["id"]: [] for im in images}
    seen = set()
    for a in data.get("annotations", []):
        aid = a.get("id")
        if aid in seen:
            raise ValueError(f"{json_file}: annotation id {aid} is not unique")
        seen.add(aid)
        if a.get("ignore", 0) != 0:
            raise ValueError(f"{json_file}: annotation {aid} has 'ignore' set; such annotations are not supported")
        if a.get("category_id") not in id_map:
            raise ValueError(f"{json_file}: annotation {aid} has category {a.get('category_id')!r}, which the file's categories do not list")
        if a.get("image_id") not in per_image:
            raise ValueError(f"{json_file}: annotation {aid} belongs to image {a.get('image_id')!r}, which the file does not list")
        bbox = a.get("bbox")
        if not (isinstance(bbox, (list, tuple)) and len(bbox) == 4 and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in bbox)):
            raise ValueError(f"{json_file}: annotation {aid} has a malformed bbox {bbox!r} (four numbers, XYWH)")
        obj = dict(bbox=[float(v) for v in bbox], bbox_mode=XYWH_ABS, iscrowd=int(a.get("iscrowd", 0)), category_id=id_map[a["category_id"]])
        obj["area"] = float(a["area"]) if "area" in a else obj["bbox"][2] * obj["bbox"][3]
        per_image[a["image_id"]].append(obj)
    records = []
    for im in images:
        rec = dict(file_name=os.path.join(image_root, im["file_name"]), image_id=im["id"], annotations=per_image[im["id"]])
        for k in ("height", "width"):
            if k in im:
                rec[k] = int(im[k])
        records.append(rec)
    return records


def register_coco_instances(name: str, metadata: dict, json_file: str, image_root: str) -> None:
    """detectron2's: the json is read on the first `DatasetCatalog.get(name)` and the records are kept"""
    cache: List[List[dict]] = []

    def load():
        if not cache:
            cache.append(load_coco_json(json_file, image_root, name))
        return cache[0]
    DatasetCatalog.register(name, load)
    meta = MetadataCatalog.get(name)
    meta.json_file, meta.image_root, meta.evaluator_type = json_file, image_root, "coco"
    for k, v in dict(metadata).items():
        setattr(meta, k, v)


def get_detection_dataset_dicts(names, filter_empty: bool = True) -> List[dict]:
    """the named datasets, concatenated; their `thing_classes` must agree; `filter_empty` drops the images that have no annotation
    with iscrowd == 0"""
    if isinstance(names, str):
        names = [names]
    names = list(names)
    if not names:
        raise ValueError("get_detection_dataset_dicts: no dataset names")
    parts = [DatasetCatalog.get(n) for n in names]
    for n, p in zip(names, parts):
        if not len(p):
            raise ValueError(f"Dataset '{n}' is empty!")
    classes = [getattr(MetadataCatalog.get(n), "thing_classes", None) for n in names]
    for n, c in zip(names, classes):
        if c != classes[0]:
            raise ValueError(f"Datasets '{names[0]}' and '{n}' have different thing_classes: {classes[0]} vs {c}")
    dicts = [r for p in parts for r in p]
    if filter_empty:
        dicts = [r for r in dicts if any(a.get("iscrowd", 0) == 0 for a in r.get("annotations", []))]
    return dicts


def all_registered(names: Sequence[str]) -> bool:
    """a non-empty list of names, each in the catalog"""
    return bool(names) and all(n in DatasetCatalog for n in names)


# the reference's datasets: name -> (json file, image root), relative to the datasets root (reference aldi/datasets.py)
REFERENCE_DATASETS = {
    "cityscapes_train": ("cityscapes/annotations/cityscapes_train_instances.json", "cityscapes/leftImg8bit/train/"),
    "cityscapes_val": ("cityscapes/annotations/cityscapes_val_instances.json", "cityscapes/leftImg8bit/val/"),
    "cityscapes_foggy_train": ("cityscapes/annotations/cityscapes_train_instances_foggyALL.json", "cityscapes/leftImg8bit_foggy/train/"),
    "cityscapes_foggy_val": ("cityscapes/annotations/cityscapes_val_instances_foggyALL.json", "cityscapes/leftImg8bit_foggy/val/"),
    "cityscapes_foggy_val_coco_ids": ("cityscapes/annotations/cityscapes_val_instances_foggyALL_coco.json", "cityscapes/leftImg8bit_foggy/val/"),
    "sim10k_cars_train": ("sim10k/coco_car_annotations.json", "sim10k/images/"),
    "cityscapes_cars_train": ("cityscapes/annotations/cityscapes_train_instances_cars.json", "cityscapes/leftImg8bit/train/"),
    "cityscapes_cars_val": ("cityscapes/annotations/cityscapes_val_instances_cars.json", "cityscapes/leftImg8bit/val/"),
    "cfc_train": ("cfc_daod/coco_labels/cfc_train.json", "cfc_daod/images/cfc_train/"),
    "cfc_val": ("cfc_daod/coco_labels/cfc_val.json", "cfc_daod/images/cfc_val/"),
    "cfc_channel_train": ("cfc_daod/coco_labels/cfc_channel_train.json", "cfc_daod/images/cfc_channel_train/"),
    "cfc_channel_test": ("cfc_daod/coco_labels/cfc_channel_test.json", "cfc_daod/images/cfc_channel_test/"),
}


def register_reference_datasets(root: str = "datasets") -> List[str]:
    """registers the dataset names the reference's configs use under `root` (names already registered are left alone); nothing is
    read until a dataset is first used.  -> the names"""
    for name, (json_file, image_root) in REFERENCE_DATASETS.items():
        if name not in DatasetCatalog:
            register_coco_instances(name, {}, os.path.join(root, json_file), os.path.join(root, image_root))
    return list(REFERENCE_DATASETS)

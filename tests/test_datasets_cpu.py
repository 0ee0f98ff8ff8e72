"""Datasets on disk, host half (aldi_amd/datasets.py, the full mapper chain of aldi_amd/aug.py): the COCO-json reader and the
catalogs, RandomCrop's draws against explicit RandomState calls, the chain's draw order, and boxes under the chain against the steps
written out.  No GPU and no image file is needed."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def catalog():
    """the process-wide catalogs, emptied of whatever the test registered"""
    from aldi_amd import datasets as D
    before_d, before_m = set(D.DatasetCatalog.list()), set(D.MetadataCatalog.list())
    yield D
    for n in set(D.DatasetCatalog.list()) - before_d:
        D.DatasetCatalog.remove(n)
    for n in set(D.MetadataCatalog.list()) - before_m:
        D.MetadataCatalog.remove(n)


def _coco(images, annotations, cats=((7, "seven"), (2, "two"), (11, "eleven"))):
    return dict(images=images, annotations=annotations, categories=[dict(id=i, name=n) for i, n in cats])


def _write(path, data):
    with open(path, "w") as f:
        json.dump(data, f)
    return str(path)


IMAGES = [dict(id=30, file_name="c.png", height=10, width=20), dict(id=10, file_name="a.png", height=12, width=8),
          dict(id=20, file_name="b.png", height=10, width=20), dict(id=40, file_name="d.png", height=10, width=20)]
ANNOS = [dict(id=1, image_id=10, category_id=7, bbox=[1, 2, 3, 4], area=12.0, iscrowd=0),
         dict(id=2, image_id=10, category_id=11, bbox=[0.5, 0.5, 2, 2], iscrowd=0),
         dict(id=3, image_id=10, category_id=2, bbox=[0, 0, 8, 12], area=96.0, iscrowd=1),
         dict(id=4, image_id=30, category_id=2, bbox=[4, 4, 5, 5], area=25.0),
         dict(id=5, image_id=40, category_id=7, bbox=[0, 0, 20, 10], area=200.0, iscrowd=1)]        # image 20: none; image 40: only a crowd


# ------------------------------------------------------------------------------------------------ json, catalogs
def test_coco_json_records_contiguous_ids_and_filter_empty(tmp_path, catalog):
    D = catalog
    jf = _write(tmp_path / "ann.json", _coco(IMAGES, ANNOS))
    assert "ds_a" not in D.DatasetCatalog
    D.register_coco_instances("ds_a", {"extra": 5}, jf, "root/dir")
    assert "ds_a" in D.DatasetCatalog and "ds_a" in D.DatasetCatalog.list()
    meta = D.MetadataCatalog.get("ds_a")
    assert meta.json_file == jf and meta.image_root == "root/dir" and meta.extra == 5 and not hasattr(meta, "thing_classes")     # lazy
    recs = D.DatasetCatalog.get("ds_a")
    assert D.DatasetCatalog.get("ds_a") is recs                                             # read once
    assert [r["image_id"] for r in recs] == [10, 20, 30, 40]
    assert [r["file_name"] for r in recs] == [os.path.join("root/dir", n) for n in ("a.png", "b.png", "c.png", "d.png")]
    assert [(r["height"], r["width"]) for r in recs] == [(12, 8), (10, 20), (10, 20), (10, 20)]
    assert meta.thing_classes == ["two", "seven", "eleven"] and meta.thing_dataset_id_to_contiguous_id == {2: 0, 7: 1, 11: 2}
    a = recs[0]["annotations"]
    assert [x["category_id"] for x in a] == [1, 2, 0] and [x["iscrowd"] for x in a] == [0, 0, 1]
    assert a[0] == dict(bbox=[1.0, 2.0, 3.0, 4.0], bbox_mode="XYWH_ABS", iscrowd=0, category_id=1, area=12.0)
    assert a[1]["area"] == 4.0                                                              # no area in the file: w * h
    assert recs[1]["annotations"] == [] and recs[2]["annotations"][0]["iscrowd"] == 0
    assert [r["image_id"] for r in D.get_detection_dataset_dicts(["ds_a"])] == [10, 30]     # none / only a crowd one: dropped
    assert [r["image_id"] for r in D.get_detection_dataset_dicts("ds_a", filter_empty=False)] == [10, 20, 30, 40]
    # concatenation, and the refusal of differing classes
    D.register_coco_instances("ds_b", {}, jf, "other")
    assert [r["file_name"].split(os.sep)[0] for r in D.get_detection_dataset_dicts(["ds_a", "ds_b"])] == ["root", "root", "other", "other"]
    jf2 = _write(tmp_path / "ann2.json", _coco(IMAGES, ANNOS[:1], cats=((7, "seven"), (2, "deux"), (11, "eleven"))))
    D.register_coco_instances("ds_c", {}, jf2, "x")
    with pytest.raises(ValueError, match="thing_classes"):
        D.get_detection_dataset_dicts(["ds_a", "ds_c"])
    with pytest.raises(ValueError, match="already registered"):
        D.register_coco_instances("ds_a", {}, jf, "x")
    with pytest.raises(KeyError, match="not registered"):
        D.DatasetCatalog.get("nope")
    D.DatasetCatalog.remove("ds_b")
    assert "ds_b" not in D.DatasetCatalog


def test_catalog_starts_empty_and_reference_names_register_lazily(catalog, tmp_path):
    D = catalog
    assert not any(n in D.DatasetCatalog for n in D.REFERENCE_DATASETS)                     # never registered at import
    names = D.register_reference_datasets(str(tmp_path / "nowhere"))                       # nothing is read: the folder does not exist
    assert {"cityscapes_train", "cityscapes_val", "cityscapes_foggy_train", "cityscapes_foggy_val", "sim10k_cars_train", "cfc_train",
            "cfc_val"} <= set(names)
    assert D.all_registered(["cityscapes_train", "cityscapes_foggy_train"]) and not D.all_registered([]) and not D.all_registered(["cityscapes_train", "x"])
    m = D.MetadataCatalog.get("cityscapes_foggy_val")
    assert m.json_file == os.path.join(str(tmp_path / "nowhere"), "cityscapes/annotations/cityscapes_val_instances_foggyALL.json")
    assert m.image_root == os.path.join(str(tmp_path / "nowhere"), "cityscapes/leftImg8bit_foggy/val/")
    with pytest.raises(FileNotFoundError):
        D.DatasetCatalog.get("cityscapes_train")
    assert D.register_reference_datasets(str(tmp_path / "nowhere")) == names               # again: left alone


@pytest.mark.parametrize("what", ["duplicate", "category", "ignore", "bbox"])
def test_each_json_error_names_its_file_and_the_id(what, tmp_path, catalog):
    annos = [dict(a) for a in ANNOS]
    if what == "duplicate":
        annos[3]["id"], match = 2, "annotation id 2 "
    elif what == "category":
        annos[1]["category_id"], match = 5, "annotation 2 .*category 5"
    elif what == "ignore":
        annos[0]["ignore"], match = 1, "annotation 1 .*ignore"
    else:
        annos[3]["bbox"], match = [1, 2, 3], "annotation 4 .*malformed bbox"
    jf = _write(tmp_path / f"bad_{what}.json", _coco(IMAGES, annos))
    with pytest.raises(ValueError, match=match) as e:
        catalog.load_coco_json(jf, "r")
    assert f"bad_{what}.json" in str(e.value)


# ------------------------------------------------------------------------------------------------ the chain's draws
def test_random_crop_draws_equal_explicit_randomstate_calls():
    from aldi_amd.aug import RandomCrop
    h, w = 96, 128
    # relative: nothing drawn for the size
    a, b = np.random.RandomState(1), np.random.RandomState(1)
    ch, cw = int(h * 0.5 + 0.5), int(w * 0.75 + 0.5)
    assert RandomCrop("relative", (0.5, 0.75)).get_params(h, w, a) == (int(b.randint(h - ch + 1)), int(b.randint(w - cw + 1)), ch, cw)
    # relative_range
    a, b = np.random.RandomState(2), np.random.RandomState(2)
    cs = np.asarray((0.3, 0.6), dtype=np.float32)
    fh, fw = cs + b.rand(2) * (1 - cs)
    ch, cw = int(h * fh + 0.5), int(w * fw + 0.5)
    assert RandomCrop("relative_range", (0.3, 0.6)).get_params(h, w, a) == (int(b.randint(h - ch + 1)), int(b.randint(w - cw + 1)), ch, cw)
    # absolute, and a crop larger than the image: clipped to it, the offsets are randint(1) == 0
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    assert RandomCrop("absolute", (48, 80)).get_params(h, w, a) == (int(b.randint(h - 48 + 1)), int(b.randint(w - 80 + 1)), 48, 80)
    assert RandomCrop("absolute", (500, 100)).get_params(h, w, a) == (int(b.randint(1)), int(b.randint(w - 100 + 1)), 96, 100)
    # absolute_range, larger than the image in one axis
    a, b = np.random.RandomState(4), np.random.RandomState(4)
    ch = int(b.randint(min(h, 90), min(h, 120) + 1))
    cw = int(b.randint(min(w, 90), min(w, 120) + 1))
    assert ch in range(90, 97) and RandomCrop("absolute_range", (90, 120)).get_params(h, w, a) == (int(b.randint(h - ch + 1)), int(b.randint(w - cw + 1)), ch, cw)
    assert a.get_state()[2] == b.get_state()[2] and np.array_equal(a.get_state()[1], b.get_state()[1])
    with pytest.raises(ValueError, match="does not fit"):
        RandomCrop("relative", (1.5, 0.5)).get_params(h, w, np.random.RandomState(0))
    with pytest.raises(ValueError, match="crop_type"):
        RandomCrop("fancy", (1, 1))


@pytest.mark.parametrize("flip", ["horizontal", "vertical"])
def test_draw_view_params_consumes_exactly_the_chains_draws(flip):
    from aldi_amd import aug
    augs = [aug.RandomCrop("absolute_range", (48, 80)), aug.ResizeShortestEdge((64, 96), 160, "choice"),
            aug.RandomFlip(0.5, horizontal=flip == "horizontal", vertical=flip == "vertical")]
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    seen = set()
    for _ in range(12):
        p = aug.draw_view_params(augs, 96, 128, a, swap_rb=True)
        ch = int(b.randint(48, 81))
        cw = int(b.randint(48, 81))
        y0 = int(b.randint(96 - ch + 1))
        x0 = int(b.randint(128 - cw + 1))
        size = int(b.choice((64, 96)))
        nh, nw = aug.ResizeShortestEdge.get_output_shape(ch, cw, size, 160)                 # of the CROPPED size
        f = bool(b.uniform(0, 1.0) < 0.5)
        assert p == aug.ViewParams(96, 128, y0, x0, ch, cw, nh, nw, hflip=f and flip == "horizontal", vflip=f and flip == "vertical", swap_rb=True)
        seen.add(f)
    assert seen == {True, False}
    assert a.get_state()[2] == b.get_state()[2] and np.array_equal(a.get_state()[1], b.get_state()[1])
    # the two-stage chain draws what draw_weak_params draws
    two = augs[1:2] + [aug.RandomFlip(0.5, horizontal=True)]
    a, b = np.random.RandomState(12), np.random.RandomState(12)
    for _ in range(6):
        assert aug.draw_view_params(two, 96, 128, a) == aug.ViewParams.whole(aug.draw_weak_params(two, 96, 128, b))
    with pytest.raises(ValueError, match="first stage"):
        aug.draw_view_params([augs[1], augs[0]], 96, 128, np.random.RandomState(0))
    with pytest.raises(ValueError, match="vertical"):
        aug.draw_weak_params([augs[1], aug.RandomFlip(0.5, horizontal=False, vertical=True)], 96, 128, np.random.RandomState(0))


def _cfg(*files):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    for f in files:
        cfg.merge_from_file(os.path.join(ROOT, "configs", f))
    return cfg


def test_get_view_augs_on_the_repositorys_configs():
    from aldi_amd import aug
    cfg = _cfg("Base-DETR.yaml")
    assert [type(a) for a in aug.get_view_augs(cfg, True)] == [aug.ResizeShortestEdge, aug.RandomFlip]      # (the file sets no crop yet)
    cfg.merge_from_list(["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "absolute_range", "INPUT.CROP.SIZE", (384, 600),
                         "INPUT.MIN_SIZE_TRAIN", (480, 512, 544, 576, 608, 640, 672, 704, 736, 768, 800)])   # the reference's Base-DETR.yaml
    train = aug.get_view_augs(cfg, True)
    assert [type(a) for a in train] == [aug.RandomCrop, aug.ResizeShortestEdge, aug.RandomFlip]
    assert (train[0].crop_type, tuple(train[0].crop_size)) == ("absolute_range", (384, 600)) and train[2].horizontal and not train[2].vertical
    assert train[1].short_edge_length[0] == 480 and train[1].short_edge_length[-1] == 800
    assert [type(a) for a in aug.get_view_augs(cfg, False)] == [aug.ResizeShortestEdge]      # no crop, no flip at test time
    with pytest.raises(ValueError, match="INPUT.CROP.ENABLED"):
        aug.get_weak_augs(cfg, True)                                                       # the two-stage entry still refuses it
    rcnn = _cfg("cityscapes/ALDI-Best-Cityscapes.yaml")
    assert [type(a) for a in aug.get_view_augs(rcnn, True)] == [aug.ResizeShortestEdge, aug.RandomFlip]
    rcnn.INPUT.RANDOM_FLIP = "vertical"
    v = aug.get_view_augs(rcnn, True)[1]
    assert v.vertical and not v.horizontal
    rcnn.INPUT.RANDOM_FLIP = "none"
    assert [type(a) for a in aug.get_view_augs(rcnn, True)] == [aug.ResizeShortestEdge]


# ------------------------------------------------------------------------------------------------ boxes
def _steps(box, p):
    """one XYXY box through the chain, written out: float64, then float32"""
    x0, y0, x1, y1 = (np.float64(v) for v in box)
    xs = [(x - p.x0) * (p.new_w * 1.0 / p.w) for x in (x0, x1)]
    ys = [(y - p.y0) * (p.new_h * 1.0 / p.h) for y in (y0, y1)]
    if p.hflip:
        xs = [p.new_w - x for x in xs]
    if p.vflip:
        ys = [p.new_h - y for y in ys]
    out = [min(xs), min(ys), max(xs), max(ys)]
    out = [max(v, 0.0) for v in out]
    out = [min(v, lim) for v, lim in zip(out, (p.new_w, p.new_h, p.new_w, p.new_h))]
    return np.array(out, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("hflip,vflip", [(False, False), (True, False), (False, True), (True, True)])
def test_boxes_under_the_chain_equal_the_steps_written_out(hflip, vflip):
    from aldi_amd import aug
    p = aug.ViewParams(96, 128, 10, 20, 50, 60, 75, 90, hflip=hflip, vflip=vflip)           # window x [20, 80), y [10, 60), scale 1.5
    boxes = np.array([[30.0, 20.0, 50.0, 40.0],        # inside
                      [5.0, 15.0, 45.5, 70.25],        # cut by the window on the left and at the bottom
                      [90.0, 70.0, 120.0, 90.0],       # wholly outside, right and below: dropped
                      [0.0, 0.0, 19.0, 9.0]])          # wholly outside, left and above: dropped
    got = aug.transform_view_boxes(boxes, p)
    assert got.dtype == np.float64
    for b, g in zip(boxes, got):
        assert np.array_equal(g.astype(np.float32), _steps(b, p)), (b, g)
    if not hflip and not vflip:
        assert got.tolist() == [[15.0, 15.0, 45.0, 45.0], [0.0, 7.5, 38.25, 75.0], [90.0, 75.0, 90.0, 75.0], [0.0, 0.0, 0.0, 0.0]]
    if hflip and vflip:
        assert got[0].tolist() == [45.0, 30.0, 75.0, 60.0]
    inst = {"image_size": (96, 128), "gt_boxes": torch.from_numpy(boxes).float(), "gt_classes": torch.tensor([3, 1, 2, 0])}
    out = aug.transform_instances(inst, p)
    assert out["image_size"] == (75, 90) and out["gt_classes"].tolist() == [3, 1] and out["gt_boxes"].dtype == torch.float32
    assert np.array_equal(out["gt_boxes"].numpy(), np.stack([_steps(boxes[0], p), _steps(boxes[1], p)]))
    # a window that covers the image: the two-stage transform, bit for bit
    w = aug.WeakParams(96, 128, 64, 85, flip=hflip)
    if not vflip:
        assert np.array_equal(aug.transform_view_boxes(boxes, aug.ViewParams.whole(w)), aug.transform_boxes(boxes, w))

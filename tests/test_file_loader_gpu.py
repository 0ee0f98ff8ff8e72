"""File-backed loaders on the device: FileDetectionLoader -> the loader stage with the FULL mapper chain (crop,
resize, vertical flip, channel order inside csrc/geom.hip) against the host restatement under the same draws, bit-exact; no host sync
in `next()`; AP 100 for a ground-truth "model" through the file-backed test loader; and, last, two trainer iterations with
DATASETS.FILES.  The dataset is six small images written to tmp_path as .ppm and .npy: no Pillow is needed."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pil_resize_ref as R  # noqa: E402

SIZES = [(96, 128)] * 4 + [(80, 100)] * 2
# two boxes per image that every 72 x 96 window of a 96 x 128 image contains whole (y0 <= 24, x0 <= 32), XYWH, and one crowd box
BOXES = [[40.0, 30.0, 50.0, 36.0], [44.5, 32.25, 20.0, 30.5]]


def _write_ppm(path, img):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())


@pytest.fixture
def dataset(tmp_path):
    """-> (name of all six, name of the four 96 x 128 ones, {image_id: raw RGB array}); registered for the test's duration"""
    from aldi_amd import datasets
    raws, images, annos = {}, [], []
    for i, (h, w) in enumerate(SIZES):
        img = np.random.RandomState(300 + i).randint(0, 256, size=(h, w, 3)).astype(np.uint8)
        fn = f"im{i}.ppm" if i % 2 == 0 else f"im{i}.npy"
        _write_ppm(str(tmp_path / fn), img) if fn.endswith(".ppm") else np.save(str(tmp_path / fn), img)
        raws[i + 1] = img
        images.append(dict(id=i + 1, file_name=fn, height=h, width=w))
        for k, b in enumerate(BOXES):
            annos.append(dict(id=len(annos) + 1, image_id=i + 1, category_id=1 + (i + k) % 3, bbox=b, iscrowd=0, area=b[2] * b[3]))
        annos.append(dict(id=len(annos) + 1, image_id=i + 1, category_id=2, bbox=[0.0, 0.0, 30.0, 30.0], iscrowd=1, area=900.0))
    cats = [dict(id=c, name=f"c{c}") for c in (1, 2, 3)]
    names = []
    for tag, keep in (("all", images), ("four", images[:4])):
        path = str(tmp_path / f"{tag}.json")
        ids = {im["id"] for im in keep}
        json.dump(dict(images=keep, annotations=[a for a in annos if a["image_id"] in ids], categories=cats), open(path, "w"))
        name = f"floader_{tag}_{tmp_path.name}"
        datasets.register_coco_instances(name, {}, path, str(tmp_path))
        names.append(name)
    yield names[0], names[1], raws
    for n in names:
        datasets.DatasetCatalog.remove(n)
        datasets.MetadataCatalog.remove(n)


def _cfg(*pairs):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SEED", 1, "AUG.DEVICE_WEAK", True, "DATASETS.FILES", True] + list(pairs))
    return cfg


CROP_CHAIN = ["INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", [0.5, 0.5], "INPUT.RANDOM_FLIP", "vertical",
              "INPUT.MIN_SIZE_TRAIN", (40, 56), "INPUT.MAX_SIZE_TRAIN", 72]
BS, STEPS, SAMPLER_SEED, W_SEED = 4, 3, 5, 12


def _stage(cfg, name, strong=None, seed=11):
    from aldi_amd import aug
    from aldi_amd.dataloader import DeviceStrongAugLoader, FileDetectionLoader, TrainingSampler
    from aldi_amd.datasets import get_detection_dataset_dicts
    from aldi_amd.mapper import DatasetMapper
    dicts = get_detection_dataset_dicts([name], filter_empty=True)
    mapper = DatasetMapper(cfg, True, True)
    files = FileDetectionLoader(dicts, mapper, BS, TrainingSampler(len(dicts), True, SAMPLER_SEED), num_threads=3)
    return DeviceStrongAugLoader(files, strong, seed, weak=aug.get_view_augs(cfg, True), weak_seed=W_SEED, view=True, swap_rb=mapper.swap_rb), files


def _sampler_stream(size, seed, count):
    g = torch.Generator()
    g.manual_seed(seed)
    out = []
    while len(out) < count:
        out += torch.randperm(size, generator=g).tolist()
    return out[:count]


def test_stage_over_files_equals_the_host_restatement_under_the_same_draws(dataset):
    from aldi_amd import aug
    name, _, raws = dataset
    cfg = _cfg("INPUT.FORMAT", "RGB", *CROP_CHAIN)
    stage, files = _stage(cfg, name)
    assert stage.view and not stage.swap_rb
    it = iter(stage)
    got = [next(it) for _ in range(STEPS)]
    augs, rng = aug.get_view_augs(cfg, True), np.random.RandomState(W_SEED)
    assert [type(a).__name__ for a in augs] == ["RandomCrop", "ResizeShortestEdge", "RandomFlip"] and augs[2].vertical
    order = _sampler_stream(6, SAMPLER_SEED, BS * STEPS)
    params = []
    for k, d in enumerate(r for b in got for r in b):
        image_id = order[k] + 1                                        # (records in ascending image id; the sampler indexes them)
        raw = raws[image_id]
        h, w = raw.shape[:2]
        p = aug.draw_view_params(augs, h, w, rng)
        params.append(p)
        assert d["image_id"] == image_id and (d["height"], d["width"]) == (h, w) and "image_raw" not in d
        ref = R.resize(np.ascontiguousarray(raw[p.y0:p.y0 + p.h, p.x0:p.x0 + p.w]), p.new_h, p.new_w)
        if p.hflip:
            ref = ref[:, ::-1]
        if p.vflip:
            ref = ref[::-1]
        ref = torch.from_numpy(np.array(ref.transpose(2, 0, 1), order="C", copy=True))
        assert d["img_weak"].is_cuda and d["image"] is d["img_weak"]
        assert torch.equal(d["img_weak"].cpu(), ref), (k, p)
        xyxy = np.array([[b[0], b[1], b[0] + b[2], b[1] + b[3]] for b in BOXES], dtype=np.float32)     # the crowd row is dropped when training
        cls = np.array([(image_id - 1 + j) % 3 for j in range(len(BOXES))], dtype=np.int64)           # category ids 1..3 -> 0..2
        boxes = aug.transform_view_boxes(xyxy, p).astype(np.float32)
        keep = ((boxes[:, 2] - boxes[:, 0]) > 1e-5) & ((boxes[:, 3] - boxes[:, 1]) > 1e-5)
        inst = d["instances"]
        assert inst["image_size"] == (p.new_h, p.new_w)
        assert inst["gt_boxes"].dtype == torch.float32 and np.array_equal(inst["gt_boxes"].numpy(), boxes[keep]), (k, p)
        assert np.array_equal(inst["gt_classes"].numpy(), cls[keep])
    assert len({(p.y0, p.x0, p.h, p.w) for p in params}) >= 2 and {p.vflip for p in params} == {False, True}
    assert not any(p.hflip for p in params) and len({(p.raw_h, p.raw_w) for p in params}) == 2
    files.close()


def test_bgr_and_rgb_differ_exactly_by_the_channel_exchange(dataset):
    name, _, _ = dataset
    a_stage, a_files = _stage(_cfg("INPUT.FORMAT", "RGB", *CROP_CHAIN), name)
    b_stage, b_files = _stage(_cfg("INPUT.FORMAT", "BGR", *CROP_CHAIN), name)
    assert not a_stage.swap_rb and b_stage.swap_rb
    a, b = next(iter(a_stage)), next(iter(b_stage))
    assert len(a) == len(b) == BS
    for x, y in zip(a, b):
        assert torch.equal(x["img_weak"].flip(0), y["img_weak"]) and not torch.equal(x["img_weak"], y["img_weak"])
        assert torch.equal(x["instances"]["gt_boxes"], y["instances"]["gt_boxes"])
    a_files.close(), b_files.close()


def test_next_does_not_wait_for_the_device_after_warm_up(dataset):
    from aldi_amd import aug
    name, _, _ = dataset
    stage, files = _stage(_cfg(*CROP_CHAIN), name, strong=aug.build_strong_augmentation(True), seed=3)
    it = iter(stage)
    for _ in range(3):
        next(it)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            mode_works = False
        except RuntimeError:
            mode_works = True                                          # positive control of the mode
        if mode_works:
            batches = [next(it) for _ in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode", "works: three next() calls ran under 'error'" if mode_works else "is not available on this build: nothing checked")
    assert mode_works
    assert all(d["image"].is_cuda and d["image"] is not d["img_weak"] for b in batches for d in b)
    torch.cuda.synchronize()
    files.close()


@pytest.mark.parametrize("device_eval", [False, True])
def test_ground_truth_model_scores_100_through_the_file_backed_test_loader(device_eval, dataset, tmp_path):
    from aldi_amd import aug
    from aldi_amd.structures import Boxes, Instances
    from aldi_amd.trainer import ALDITrainer
    name, _, raws = dataset
    cfg = _cfg("INPUT.MIN_SIZE_TEST", 64, "INPUT.MAX_SIZE_TEST", 100, "TEST.DEVICE_EVAL", device_eval, "DATASETS.TEST", (name,), *CROP_CHAIN)
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    assert cfg.INPUT.FORMAT == "BGR"
    loader, records = ALDITrainer.build_test_loader(cfg, name)
    assert len(loader) == 6 and len(records) == 6 and not isinstance(loader, list)
    new_size = {(96, 128): (64, 85), (80, 100): (64, 80)}
    seen = []
    for b in loader:                                                   # no crop, no flip, nothing drawn at test time; BGR = channels exchanged
        (d,) = b
        raw = raws[d["image_id"]]
        nh, nw = new_size[raw.shape[:2]]
        assert d["image"].is_cuda and (d["height"], d["width"]) == raw.shape[:2]
        ref = R.resize(raw, nh, nw)[:, :, ::-1]
        assert torch.equal(d["image"].cpu(), torch.from_numpy(np.array(ref.transpose(2, 0, 1), order="C", copy=True))), d["image_id"]
        seen.append(d["image_id"])
    assert seen == [1, 2, 3, 4, 5, 6]
    by_id = {r["image_id"]: r for r in records}

    class GroundTruthModel:                                            # every annotation, in the RESIZED frame, as a confident detection
        training = False

        def eval(self):
            return self

        def train(self, mode=True):
            return self

        def __call__(self, inputs):
            out = []
            for d in inputs:
                r = by_id[d["image_id"]]
                nh, nw = (int(s) for s in d["image"].shape[1:])
                p = aug.ViewParams(r["height"], r["width"], 0, 0, r["height"], r["width"], nh, nw)
                inst = Instances((nh, nw))
                gt = np.array([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in r["annotations"]])
                inst.pred_boxes = Boxes(torch.from_numpy(aug.transform_view_boxes(gt, p)).to(torch.float32))
                inst.scores = torch.linspace(0.99, 0.5, len(gt))
                inst.pred_classes = torch.tensor([a["category_id"] for a in r["annotations"]], dtype=torch.int64)
                out.append(inst)
            return out
    res = ALDITrainer.test(cfg, GroundTruthModel())
    assert res["bbox"]["AP"] == pytest.approx(100.0) and res["bbox"]["AP50"] == pytest.approx(100.0), res


# ------------------------------------------------------------------------------------------------ the trainer (last; run in a GPU call of its own)
def test_trainer_runs_two_iterations_on_files(dataset, monkeypatch, tmp_path):
    """MIN_SIZE_TRAIN (64, 96), MAX 160 and an absolute 72 x 96 crop of the 96 x 128 images: the network's input shapes are (64, 85) and
    (96, 128), the shapes tests/test_weak_aug_gpu.py's trainer test runs"""
    from aldi_amd import aug
    from aldi_amd import dataloader as dl
    from aldi_amd.trainer import ALDITrainer
    _, four, _ = dataset
    cfg = _cfg("AUG.DEVICE_STRONG", True, "INPUT.MIN_SIZE_TRAIN", (64, 96), "INPUT.MAX_SIZE_TRAIN", 160, "INPUT.CROP.ENABLED", True,
               "INPUT.CROP.TYPE", "absolute", "INPUT.CROP.SIZE", (72, 96), "DATASETS.TRAIN", (four,), "DATASETS.UNLABELED", (four,),
               "DATALOADER.NUM_WORKERS", 2)
    cfg.OUTPUT_DIR = str(tmp_path / "out")
    seen, real_iter = [], dl.WeakStrongDataloader.__iter__

    def recording(self):
        for parts in real_iter(self):
            seen.append(parts)
            yield parts
    monkeypatch.setattr(dl.WeakStrongDataloader, "__iter__", recording)
    random.seed(4)
    torch.manual_seed(17)
    tr = ALDITrainer(cfg)
    for it in range(2):
        tr.iter = it
        tr.before_step()
        tr.run_step()
        tr.after_step()
    torch.cuda.synchronize()
    ld = {k: float(v) for k, v in tr._trainer.last_loss_dict.items()}
    assert ld and all(np.isfinite(v) for v in ld.values()), ld
    assert len(seen) >= 2
    augs = aug.get_view_augs(cfg, True)
    rngs = {lab: np.random.RandomState(dl.device_weak_seed(1, 0, lab)) for lab in (True, False)}
    sizes, windows = set(), set()
    for lw, ls, uw, us in seen:
        for lab, weak_part, strong_part in ((True, lw, ls), (False, uw, us)):
            part = strong_part if strong_part is not None else weak_part
            for i, d in enumerate(part):
                p = aug.draw_view_params(augs, 96, 128, rngs[lab], swap_rb=True)
                assert (p.h, p.w) == (72, 96) and (p.new_h, p.new_w) in ((64, 85), (96, 128))
                sizes.add((p.new_h, p.new_w))
                windows.add((p.y0, p.x0))
                assert tuple(d["image"].shape) == (3, p.new_h, p.new_w) and d["image"].is_cuda, (lab, i)
                assert d["instances"]["image_size"] == (p.new_h, p.new_w) and (d["height"], d["width"]) == (96, 128)
                if lab:                                                # (the step has replaced the unlabeled instances by the teacher's labels)
                    assert len(d["instances"]["gt_boxes"]) == len(BOXES)                   # every window holds both boxes whole
    assert len(sizes) == 2 and len(windows) > 1                        # both shapes occurred

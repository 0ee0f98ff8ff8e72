"""Host half of the file-backed loaders: `read_image` and the mapper (aldi_amd/mapper.py), the samplers and
`FileDetectionLoader` (aldi_amd/dataloader.py) with the rules that keep it from hanging -- threads only, every wait limited, errors and
stalls surfacing from `next()` with the file's name, a training stream that never ends, threads gone after `close()` -- and the
configuration behind DATASETS.FILES.  No GPU."""
import itertools
import json
import os
import re
import threading
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def write_ppm(path, img, comment=False):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"P6\n" + (b"# a comment 12 34\n" if comment else b"") + b"%d %d\n255\n" % (w, h) + img.tobytes())


def _have_pillow():
    try:
        import PIL  # noqa: F401
        return True
    except ImportError:
        return False


# ------------------------------------------------------------------------------------------------ read_image
def test_read_image_npy_and_ppm_need_numpy_only(tmp_path):
    from aldi_amd.mapper import read_image
    a, b = _img(7, 11, 1), _img(5, 3, 2)
    np.save(tmp_path / "a.npy", a)
    write_ppm(tmp_path / "b.ppm", b)
    write_ppm(tmp_path / "c.PPM", b, comment=True)
    got, swap = read_image(str(tmp_path / "a.npy"), "BGR")
    assert swap is True and got.dtype == np.uint8 and np.array_equal(got, a)                       # RGB order kept: the device exchanges
    got, swap = read_image(str(tmp_path / "b.ppm"), "RGB")
    assert swap is False and got.shape == (5, 3, 3) and np.array_equal(got, b) and got.flags.writeable
    assert np.array_equal(read_image(str(tmp_path / "c.PPM"), "RGB")[0], b)
    with pytest.raises(ValueError, match="neither 'RGB' nor 'BGR'"):
        read_image(str(tmp_path / "a.npy"), "L")


def test_read_image_other_formats_go_through_pillow_or_say_so(tmp_path, monkeypatch):
    from aldi_amd import mapper
    a = _img(6, 9, 3)
    path = str(tmp_path / "a.png")
    if _have_pillow():
        from PIL import Image
        Image.fromarray(a).save(path)
        got, swap = mapper.read_image(path, "BGR")
        assert swap and got.dtype == np.uint8 and np.array_equal(got, a) and got.flags.writeable
        Image.fromarray(a[:, :, 0]).save(str(tmp_path / "g.png"))                                 # a gray file comes back as three channels
        assert np.array_equal(mapper.read_image(str(tmp_path / "g.png"), "RGB")[0], np.repeat(a[:, :, :1], 3, axis=2))
        ex = Image.Exif()
        ex[0x0112] = 6                                                                           # stored pixels are to be turned by 270 degrees
        Image.fromarray(a).save(str(tmp_path / "r.jpg"), exif=ex, quality=100)
        assert mapper.read_image(str(tmp_path / "r.jpg"), "RGB")[0].shape == (9, 6, 3)
        with open(tmp_path / "bad.png", "wb") as f:
            f.write(open(path, "rb").read()[:40])
        with pytest.raises(ValueError, match=re.escape(str(tmp_path / "bad.png"))):
            mapper.read_image(str(tmp_path / "bad.png"), "RGB")
    # without Pillow: the named ImportError (simulated where Pillow is installed by making its import fail)
    import builtins
    real = builtins.__import__

    def no_pil(name, *args, **kw):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError("No module named 'PIL'")
        return real(name, *args, **kw)
    open(path, "ab").close()
    monkeypatch.setattr(builtins, "__import__", no_pil)
    with pytest.raises(ImportError) as e:
        mapper.read_image(path, "RGB")
    assert path in str(e.value) and ".npy" in str(e.value) and ".ppm" in str(e.value) and "Pillow" in str(e.value)


def test_truncated_and_mis_sized_files_raise_a_value_error_that_names_the_file(tmp_path):
    from aldi_amd.mapper import read_image
    b = _img(5, 3, 2)
    write_ppm(tmp_path / "ok.ppm", b)
    blob = open(tmp_path / "ok.ppm", "rb").read()
    cases = {"short.ppm": blob[:-7], "long.ppm": blob + b"\0", "head.ppm": blob[:5], "p5.ppm": b"P5" + blob[2:],
             "deep.ppm": blob.replace(b"255", b"65535", 1), "empty.ppm": b""}
    for name, data in cases.items():
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        with pytest.raises(ValueError, match=re.escape(path)):
            read_image(path, "RGB")
    with pytest.raises(ValueError, match="truncated"):
        read_image(str(tmp_path / "short.ppm"), "RGB")
    np.save(tmp_path / "f.npy", b.astype(np.float32))
    np.save(tmp_path / "g.npy", b[:, :, 0])
    np.save(tmp_path / "ok.npy", b)
    open(tmp_path / "cut.npy", "wb").write(open(tmp_path / "ok.npy", "rb").read()[:-9])
    for name in ("f.npy", "g.npy", "cut.npy"):
        with pytest.raises(ValueError, match=re.escape(str(tmp_path / name))):
            read_image(str(tmp_path / name), "RGB")
    with pytest.raises(FileNotFoundError):
        read_image(str(tmp_path / "nothing.ppm"), "RGB")


# ------------------------------------------------------------------------------------------------ the mapper
def _cfg(*pairs):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SEED", 1] + list(pairs))
    return cfg


def _record(tmp_path, h=12, w=16, name="im.npy", **kw):
    path = str(tmp_path / name)
    img = _img(h, w, 5)
    np.save(path, img) if name.endswith(".npy") else write_ppm(path, img)
    rec = dict(file_name=path, image_id=41, height=h, width=w, annotations=[
        dict(bbox=[1.5, 2.0, 4.0, 5.25], bbox_mode="XYWH_ABS", iscrowd=0, category_id=3, area=21.0),
        dict(bbox=[0.0, 0.0, 16.0, 12.0], bbox_mode="XYWH_ABS", iscrowd=1, category_id=1, area=192.0),
        dict(bbox=[7.0, 3.0, 2.0, 2.0], bbox_mode="XYWH_ABS", iscrowd=0, category_id=0, area=4.0)])
    rec.update(kw)
    return rec, img


def test_mapper_keys_dtypes_crowd_rows_and_the_unlabeled_form(tmp_path):
    from aldi_amd.mapper import DatasetMapper
    rec, img = _record(tmp_path)
    before = json.dumps(rec, sort_keys=True)
    m = DatasetMapper(_cfg(), True, True)
    assert m.swap_rb is True and DatasetMapper(_cfg("INPUT.FORMAT", "RGB"), True, True).swap_rb is False       # INPUT.FORMAT "BGR" is the default
    out = m(rec)
    assert set(out) == {"image_raw", "file_name", "image_id", "height", "width", "instances"}
    raw = out["image_raw"]
    assert raw.dtype == torch.uint8 and tuple(raw.shape) == (12, 16, 3) and not raw.is_cuda and not raw.is_pinned()
    assert np.array_equal(raw.numpy(), img)                                                       # RGB order, no geometry
    assert (out["file_name"], out["image_id"], out["height"], out["width"]) == (rec["file_name"], 41, 12, 16)
    inst = out["instances"]
    assert set(inst) == {"image_size", "gt_boxes", "gt_classes"} and inst["image_size"] == (12, 16)
    assert inst["gt_boxes"].dtype == torch.float32 and inst["gt_classes"].dtype == torch.int64
    assert inst["gt_boxes"].tolist() == [[1.5, 2.0, 5.5, 7.25], [7.0, 3.0, 9.0, 5.0]] and inst["gt_classes"].tolist() == [3, 0]   # crowd row dropped
    assert json.dumps(rec, sort_keys=True) == before                                               # the catalog's record is not modified
    test_time = DatasetMapper(_cfg(), False, True)(rec)["instances"]
    assert test_time["gt_classes"].tolist() == [3, 1, 0]                                           # only training drops crowds
    unl = DatasetMapper(_cfg(), True, False)(rec)
    assert tuple(unl["instances"]["gt_boxes"].shape) == (0, 4) and unl["instances"]["gt_boxes"].dtype == torch.float32
    assert tuple(unl["instances"]["gt_classes"].shape) == (0,) and unl["instances"]["gt_classes"].dtype == torch.int64
    assert np.array_equal(unl["image_raw"].numpy(), img)


def test_a_record_whose_size_disagrees_with_the_file_raises_naming_both(tmp_path):
    from aldi_amd.mapper import DatasetMapper
    rec, _ = _record(tmp_path, height=16, width=12)
    with pytest.raises(ValueError) as e:
        DatasetMapper(_cfg(), True, True)(rec)
    assert "12x16" in str(e.value) and "16x12" in str(e.value) and rec["file_name"] in str(e.value)
    rec, _ = _record(tmp_path)
    del rec["height"], rec["width"]
    out = DatasetMapper(_cfg(), True, True)(rec)
    assert (out["height"], out["width"]) == (12, 16)


# ------------------------------------------------------------------------------------------------ samplers
def _restated_training_stream(size, seed, rank, world, count, shuffle=True):
    """one generator, a randperm per epoch, the rank stride -- written out"""
    g = torch.Generator()
    g.manual_seed(seed)
    stream = []
    while len(stream) < rank + world * count:
        stream += (torch.randperm(size, generator=g) if shuffle else torch.arange(size)).tolist()
    return stream[rank::world][:count]


def test_training_sampler_equals_the_restatement():
    from aldi_amd.dataloader import TrainingSampler
    for size, seed, world in ((7, 3, 1), (5, 11, 2), (1, 0, 1), (10, 99, 3)):
        for rank in range(world):
            got = list(itertools.islice(iter(TrainingSampler(size, True, seed, rank, world)), 4 * size + 3))
            assert got == _restated_training_stream(size, seed, rank, world, 4 * size + 3), (size, seed, rank, world)
    assert list(itertools.islice(iter(TrainingSampler(3, False, 5)), 7)) == [0, 1, 2, 0, 1, 2, 0]
    a, b = (list(itertools.islice(iter(TrainingSampler(8, True, 21, r, 2)), 4)) for r in (0, 1))
    assert not set(a) & set(b) and sorted(a + b) == list(range(8))                                 # disjoint within the epoch, together all of it
    s = TrainingSampler(6, True, 4)
    assert list(itertools.islice(iter(s), 9)) == list(itertools.islice(iter(s), 9))                # a fresh generator per iteration
    for bad in (0, -1):
        with pytest.raises(ValueError, match="size"):
            TrainingSampler(bad)
    with pytest.raises(ValueError, match="rank"):
        TrainingSampler(4, rank=2, world=2)


def test_inference_sampler_shards_are_contiguous_and_cover():
    from aldi_amd.dataloader import InferenceSampler
    assert [list(InferenceSampler(10, r, 3)) for r in range(3)] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]]
    assert [len(InferenceSampler(10, r, 3)) for r in range(3)] == [4, 3, 3]
    assert [list(InferenceSampler(2, r, 4)) for r in range(4)] == [[0], [1], [], []]
    assert list(InferenceSampler(5)) == [0, 1, 2, 3, 4] and list(InferenceSampler(0)) == []


# ------------------------------------------------------------------------------------------------ the loader
def _dataset(tmp_path, n=3):
    dicts = []
    for i in range(n):
        path = str(tmp_path / (f"im{i}.npy" if i % 2 else f"im{i}.ppm"))
        img = _img(6 + i, 8, 50 + i)
        np.save(path, img) if path.endswith(".npy") else write_ppm(path, img)
        dicts.append(dict(file_name=path, image_id=i, height=6 + i, width=8, annotations=[dict(bbox=[1, 1, 3, 3], bbox_mode="XYWH_ABS", iscrowd=0, category_id=i)]))
    return dicts


def test_three_images_at_batch_size_four_never_stop(tmp_path):
    from aldi_amd.dataloader import FileDetectionLoader, TrainingSampler
    from aldi_amd.mapper import DatasetMapper
    dicts = _dataset(tmp_path)
    ld = FileDetectionLoader(dicts, DatasetMapper(_cfg(), True, True), 4, TrainingSampler(3, True, 9), num_threads=2)
    it = iter(ld)
    batches = [next(it) for _ in range(10)]
    ids = [r["image_id"] for b in batches for r in b]
    assert all(len(b) == 4 for b in batches) and ids == _restated_training_stream(3, 9, 0, 1, 40)  # the sampler's order, wrapped
    for b in batches[:2]:
        for r in b:
            assert np.array_equal(r["image_raw"].numpy(), _img(6 + r["image_id"], 8, 50 + r["image_id"])) and r["instances"]["gt_classes"].tolist() == [r["image_id"]]
    with pytest.raises(TypeError):
        len(ld)
    ld.close()


def test_inference_loader_is_finite_with_a_short_last_batch(tmp_path):
    from aldi_amd.dataloader import FileDetectionLoader, InferenceSampler
    from aldi_amd.mapper import DatasetMapper
    dicts = _dataset(tmp_path, 5)
    ld = FileDetectionLoader(dicts, DatasetMapper(_cfg(), False, True), 2, InferenceSampler(5), num_threads=3)
    assert len(ld) == 3
    for _ in range(2):                                                                             # iterable again
        assert [[r["image_id"] for r in b] for b in ld] == [[0, 1], [2, 3], [4]]
    assert [[r["image_id"] for r in b] for b in FileDetectionLoader(dicts, ld.mapper, 2, InferenceSampler(5, 1, 2))] == [[3, 4]]
    assert FileDetectionLoader(dicts, ld.mapper, 1, InferenceSampler(5), num_threads=999).num_threads == 16       # capped
    assert FileDetectionLoader(dicts, ld.mapper, 1, InferenceSampler(5), num_threads=0).num_threads == 1
    ld.close()


def test_a_file_that_fails_to_decode_surfaces_from_next_with_its_name(tmp_path):
    from aldi_amd.dataloader import FileDetectionLoader, TrainingSampler
    from aldi_amd.mapper import DatasetMapper
    dicts = _dataset(tmp_path)
    bad = dicts[1]["file_name"]
    open(bad, "wb").write(open(bad, "rb").read()[:50])
    it = iter(FileDetectionLoader(dicts, DatasetMapper(_cfg(), True, True), 3, TrainingSampler(3, False), num_threads=2))
    with pytest.raises(ValueError, match=re.escape(bad)):
        next(it)
    with pytest.raises(ValueError, match=re.escape(bad)):                                          # the stream goes on: the next batch holds it again
        next(it)

    def stops(rec):                                                                                # a StopIteration on the thread must not end the stream
        raise StopIteration
    it = iter(FileDetectionLoader(dicts, stops, 2, TrainingSampler(3, False), num_threads=1))
    with pytest.raises(RuntimeError, match=re.escape(dicts[0]["file_name"])):
        next(it)


def test_a_stalled_decode_is_a_named_timeout_not_a_stall(tmp_path):
    from aldi_amd import dataloader as dl
    from aldi_amd.mapper import DatasetMapper
    assert dl.DECODE_TIMEOUT_S == 120.0
    dicts = _dataset(tmp_path)
    release, mapper = threading.Event(), DatasetMapper(_cfg(), True, True)

    def slow(rec):
        if rec["image_id"] == 1:
            release.wait(20)                                                                       # (released below; bounded whatever happens)
        return mapper(rec)
    ld = dl.FileDetectionLoader(dicts, slow, 3, dl.TrainingSampler(3, False), num_threads=2, timeout=0.05)
    assert dl.FileDetectionLoader(dicts, slow, 3, dl.TrainingSampler(3, False)).timeout == 120.0
    t0 = time.monotonic()
    try:
        with pytest.raises(TimeoutError, match=re.escape(dicts[1]["file_name"])):
            next(iter(ld))
        assert time.monotonic() - t0 < 5
    finally:
        release.set()
        ld.close()


def test_close_returns_the_thread_count_to_its_baseline(tmp_path):
    from aldi_amd.dataloader import FileDetectionLoader, TrainingSampler
    from aldi_amd.mapper import DatasetMapper
    dicts = _dataset(tmp_path)
    deadline = time.monotonic() + 5                                                                # (decode threads of earlier tests' loaders are on their way out)
    while any(t.name.startswith("aldi-decode") for t in threading.enumerate()) and time.monotonic() < deadline:
        time.sleep(0.01)
    base = threading.active_count()
    ld = FileDetectionLoader(dicts, DatasetMapper(_cfg(), True, True), 4, TrainingSampler(3), num_threads=4)
    it = iter(ld)
    next(it), next(it)
    assert threading.active_count() > base
    ld.close()                                                                                     # with a look-ahead batch outstanding
    deadline = time.monotonic() + 5
    while threading.active_count() > base and time.monotonic() < deadline:
        time.sleep(0.01)
    assert threading.active_count() == base
    # dropping the loader does the same through __del__
    ld = FileDetectionLoader(dicts, DatasetMapper(_cfg(), True, True), 2, TrainingSampler(3), num_threads=2)
    next(iter(ld))
    del ld
    deadline = time.monotonic() + 5
    while threading.active_count() > base and time.monotonic() < deadline:
        time.sleep(0.01)
    assert threading.active_count() == base


# ------------------------------------------------------------------------------------------------ configuration
def test_datasets_files_defaults_to_off_and_off_builds_the_loaders_of_before():
    from aldi_amd.dataloader import DeviceStrongAugLoader, SyntheticDetectionLoader, WeakStrongDataloader
    from aldi_amd.trainer import ALDITrainer
    cfg = _cfg("DATASETS.TRAIN", ("cityscapes_train",), "DATASETS.UNLABELED", ("cityscapes_foggy_train",))
    assert cfg.DATASETS.FILES is False and cfg.DATASETS.TRAIN                                     # names are set, the loaders stay synthetic
    off = ALDITrainer.build_train_loader(cfg)
    assert type(off) is WeakStrongDataloader and type(off.labeled_loader) is SyntheticDetectionLoader and type(off.unlabeled_loader) is SyntheticDetectionLoader
    s = ALDITrainer.build_train_loader(_cfg("AUG.DEVICE_STRONG", True, "AUG.DEVICE_WEAK", True))
    assert type(s.labeled_loader) is DeviceStrongAugLoader and type(s.labeled_loader.loader) is SyntheticDetectionLoader
    assert s.labeled_loader.view is False and s.labeled_loader.swap_rb is False                    # get_weak_augs: the two-stage path
    batches, records = ALDITrainer.build_test_loader(_cfg("SYNTHETIC.HEIGHT", 32, "SYNTHETIC.WIDTH", 48, "SYNTHETIC.VAL_IMAGES", 2), "synthetic_val")
    assert isinstance(batches, list) and len(batches) == 2 and not batches[0][0]["image"].is_cuda


def test_files_without_device_weak_raises_naming_both_keys():
    from aldi_amd.trainer import ALDITrainer
    for build in (ALDITrainer.build_train_loader, lambda c: ALDITrainer.build_test_loader(c, "whatever")):
        with pytest.raises(ValueError) as e:
            build(_cfg("DATASETS.FILES", True))
        assert "DATASETS.FILES" in str(e.value) and "AUG.DEVICE_WEAK" in str(e.value)


def test_unregistered_dataset_names_raise_listing_them(tmp_path):
    from aldi_amd import datasets
    from aldi_amd.trainer import ALDITrainer
    cfg = _cfg("DATASETS.FILES", True, "AUG.DEVICE_WEAK", True, "DATASETS.TRAIN", ("floader_known", "floader_missing_a"),
               "DATASETS.UNLABELED", ("floader_missing_b",), "DATASETS.TEST", ("floader_missing_c",))
    datasets.register_coco_instances("floader_known", {}, str(tmp_path / "none.json"), str(tmp_path))
    try:
        with pytest.raises(KeyError) as e:
            ALDITrainer.build_train_loader(cfg)
        assert "floader_missing_a" in str(e.value) and "floader_missing_b" in str(e.value) and "'floader_known'" not in str(e.value).split("registered")[0]
        with pytest.raises(KeyError, match="floader_missing_c"):
            ALDITrainer.build_test_loader(cfg, "floader_missing_c")
        assert "floader_missing_a" not in datasets.DatasetCatalog                                  # nothing is registered implicitly
    finally:
        datasets.DatasetCatalog.remove("floader_known")
        datasets.MetadataCatalog.remove("floader_known")


def test_stage_recognises_the_full_chain_and_keeps_the_weak_path():
    from aldi_amd import aug
    from aldi_amd.dataloader import DeviceStrongAugLoader
    weak = [aug.ResizeShortestEdge((40,), 72, "choice"), aug.RandomFlip(0.5, horizontal=True)]
    assert DeviceStrongAugLoader([], None, 1, weak=weak).view is False
    assert DeviceStrongAugLoader([], None, 1, weak=weak, view=True, swap_rb=True).swap_rb is True
    assert DeviceStrongAugLoader([], None, 1, weak=[aug.RandomCrop("relative", (0.5, 0.5))] + weak).view is True
    assert DeviceStrongAugLoader([], None, 1, weak=[weak[0], aug.RandomFlip(0.5, horizontal=False, vertical=True)]).view is True
    assert DeviceStrongAugLoader([], None, 1).view is False
    with pytest.raises(ValueError, match="view=True"):
        DeviceStrongAugLoader([], None, 1, weak=weak, swap_rb=True)
    with pytest.raises(ValueError, match="need the chain"):
        DeviceStrongAugLoader([], None, 1, view=True)


def test_the_new_modules_import_no_worker_process_machinery():
    for name in ("mapper.py", "dataloader.py"):
        src = open(os.path.join(ROOT, "aldi_amd", name)).read()
        imports = re.findall(r"^\s*(?:from|import)\s+([\w.]+)", src, flags=re.M)
        assert imports and not [m for m in imports if m.split(".")[0] == "multiprocessing" or m.startswith("torch.utils.data") or m.startswith("torch.multiprocessing")], name
        assert "os.cpu_count" not in src and "DataLoader(" not in src and "os.fork" not in src
    src = open(os.path.join(ROOT, "aldi_amd", "mapper.py")).read()
    assert not re.search(r"\.cuda\b|pin_memory\(|\.to\(|torch\.cuda", src)                         # a decode thread makes no device call


def test_train_net_arguments_and_dataset_root(tmp_path):
    import importlib.util
    from aldi_amd import datasets
    spec = importlib.util.spec_from_file_location("train_net_tool", os.path.join(ROOT, "tools", "train_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    config = os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml")
    a = tool.parse_args(["--config-file", config, "--eval-only", "--resume", "SOLVER.IMS_PER_BATCH", "4", "DATASETS.TEST", '("cityscapes_val",)'])
    assert a.eval_only and a.resume and a.dataset_root is None and a.opts[:2] == ["SOLVER.IMS_PER_BATCH", "4"]
    before = set(datasets.DatasetCatalog.list())
    cfg = tool.setup(a)
    assert cfg.DATASETS.FILES is False and cfg.SOLVER.IMS_PER_BATCH == 4 and tuple(cfg.DATASETS.TEST) == ("cityscapes_val",)
    assert set(datasets.DatasetCatalog.list()) == before                                           # without --dataset-root nothing is registered
    try:
        cfg = tool.setup(tool.parse_args(["--config-file", config, "--dataset-root", str(tmp_path), "AUG.DEVICE_STRONG", "True"]))
        assert cfg.DATASETS.FILES is True and cfg.AUG.DEVICE_WEAK is True and cfg.AUG.DEVICE_STRONG is True
        assert set(datasets.REFERENCE_DATASETS) <= set(datasets.DatasetCatalog.list())
        assert datasets.MetadataCatalog.get("cityscapes_train").json_file.startswith(str(tmp_path))
    finally:
        for n in set(datasets.DatasetCatalog.list()) - before:
            datasets.DatasetCatalog.remove(n)
            datasets.MetadataCatalog.remove(n)

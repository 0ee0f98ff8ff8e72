"""Batched strong views (aldi_amd/aug.py strong_views -> csrc/aug.hip batch_sums / fill / view kernels) and the loader stage
(aldi_amd/dataloader.py DeviceStrongAugLoader, AUG.DEVICE_STRONG): byte-identical to the per-op chain, to the oracle and to
golden g9, with the same generator consumption.  Every comparison is bit-exact."""
import itertools
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(H, W, seed):
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[: H // 4] = 250                                   # saturating band
    return img


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _chain(erasing=True, mic=None):
    from aldi_amd import aug
    augs = aug.build_strong_augmentation(include_erasing=erasing)
    if mic is not None:
        augs.append(aug.RandomApply(aug.MICTransform(*mic), prob=1.0))
    return augs


def _per_op(imgs_hwc, augs):
    """the per-op kernels, image by image, consuming the global streams (the chain's `apply_image`s)"""
    from aldi_amd import aug
    outs = []
    for im in imgs_hwc:
        x = dev(im)
        for a in augs:
            x = a.apply_image(x)
        outs.append(x.cpu().numpy())
    return outs


SIZES = [(5, 7), (17, 9), (64, 96), (211, 333), (800, 1333), (1024, 2048), (31, 130), (100, 65)]


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("mic", [None, (0.5, 4)])
def test_ragged_batch_equals_sequential_per_op_chain(n, mic):
    from aldi_amd import aug
    augs = _chain(True, mic)
    for seed in range(3):
        sizes = [SIZES[(seed * 3 + i) % len(SIZES)] for i in range(n)]
        imgs = [_img(H, W, 10 * seed + i) for i, (H, W) in enumerate(sizes)]
        np.random.seed(seed); random.seed(seed)
        ref = _per_op(imgs, augs)
        st_np, st_py = np.random.get_state(), random.getstate()
        np.random.seed(seed); random.seed(seed)
        out = aug.strong_views([dev(i.transpose(2, 0, 1)) for i in imgs], augs, chw=True)
        assert np.array_equal(np.random.get_state()[1], st_np[1]) and np.random.get_state()[2] == st_np[2]
        assert random.getstate() == st_py
        for i, (o, r) in enumerate(zip(out, ref)):
            assert np.array_equal(o.cpu().numpy(), r.transpose(2, 0, 1)), (seed, i, sizes[i])


SIGMAS = [0.1, 0.124, 0.9, 2.0]


def test_forced_parameters_every_gate_combination_vs_oracle():
    """colour / grayscale / blur / erase / MIC gates in all 32 combinations, sigma radius 0..8, overlapping erase rects on all four
    borders, MIC blocks 16/32/64 on sizes they do not divide"""
    from aldi_amd import aug
    from oracle import aug_ops as ao
    H, W = 203, 317
    img = _img(H, W, 5)
    rects = [(0, 0, 60, 90), (40, 60, 163, 80), (150, 250, 53, 67)]       # top-left; bottom border, overlaps the first; bottom-right
    rects2 = [(0, 200, 30, 117), (10, 0, 50, 40)]                          # right border; left border
    views, params, refs = [], [], []
    for k, (c, g, b, e, m) in enumerate(itertools.product([0, 1], repeat=5)):
        rs = np.random.RandomState(k)
        erases, ops_ = [], []
        p = aug.StrongParams(H, W)
        if c:
            p.colour = (0.6 + 0.02 * k, 1.4 - 0.01 * k, 0.7 + 0.015 * k)
            ops_ += [("contrast", p.colour[0]), ("brightness", p.colour[1]), ("saturation", p.colour[2])]
        if g:
            p.gray = 0.0 if k % 3 else 0.25
            ops_.append(("saturation", p.gray))
        if b:
            p.sigma = SIGMAS[k % 4]
            ops_.append(("blur", p.sigma))
        if e:
            for rect in (rects if k % 2 else rects2):
                ref_rs = np.random.RandomState(); ref_rs.set_state(rs.get_state())
                snaps, pos = aug.np_mt_advance(rs, 2 * rect[2] * rect[3] * 3)
                p.erases.append((rect, snaps, pos))
                ops_.append(("erase", rect, ref_rs.rand(rect[2], rect[3], 3)))
        if m:
            block = (16, 32, 64)[k % 3]
            p.mic = rs.rand(*ao.mic_grid(H, W, block)) > 0.5
            ops_.append(("mic", p.mic))
        views.append(dev(img.transpose(2, 0, 1)))
        params.append(p)
        refs.append(ao.apply_ops(img, ops_))
    out = aug.launch_strong_views(views, params, chw=True)
    for k, (o, r) in enumerate(zip(out, refs)):
        assert np.array_equal(o.cpu().numpy(), r.transpose(2, 0, 1)), (k, [x[0] for x in params[k].ops()])


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", [(5, 7), (9, 70), (33, 129)])
def test_blur_on_images_smaller_than_the_window(sigma, shape):
    from aldi_amd import aug
    from oracle import aug_ops as ao
    img = _img(*shape, 1)
    out = aug.launch_strong_views([dev(img)], [aug.StrongParams(*shape, sigma=sigma)], chw=False)[0]
    assert np.array_equal(out.cpu().numpy(), ao.gaussian_blur(img, sigma))


def test_golden_g9_through_the_batched_path():
    from aldi_amd import aug
    g9 = np.load(os.path.join(ROOT, "tests", "golden", "g9_aug.npz"))
    for tag in ("a", "b"):
        img = g9[f"img_{tag}"]
        H, W, _ = img.shape
        d = dev(img)
        for i in range(3):
            random.seed(int(g9[f"blur_{tag}{i}_seed"]))
            out = aug.strong_views([d], [aug.RandomApply(aug.RandomBlurTransform((0.1, 2.0)), prob=1.0)], chw=False,
                                   np_rng=np.random.RandomState(0))[0]
            assert np.array_equal(out.cpu().numpy(), g9[f"blur_{tag}{i}"]), ("blur", tag, i)
        for i in range(3):
            seed, sl, sh, r1, r2 = g9[f"erase_{tag}{i}_cfg"]
            random.seed(int(seed))
            np.random.seed(int(seed))
            rect = aug.RandomEraseTransform(sl=sl, sh=sh, r1=r1, r2=r2).draw(H, W)
            snaps, pos = aug.np_mt_advance(np.random, 2 * rect[2] * rect[3] * 3)
            out = aug.launch_strong_views([d], [aug.StrongParams(H, W, erases=[(rect, snaps, pos)])], chw=False)[0]
            assert np.array_equal(out.cpu().numpy(), g9[f"erase_{tag}{i}"]), ("erase", tag, i)
        for i in range(2):
            seed, ratio, block = g9[f"mic_{tag}{i}_cfg"]
            np.random.seed(int(seed))
            out = aug.strong_views([d], [aug.RandomApply(aug.MICTransform(ratio, int(block)), prob=1.0)], chw=False,
                                   np_rng=np.random.RandomState(0))[0]
            np.random.seed(int(seed))
            mask = np.random.rand(round(H / int(block)), round(W / int(block))) > ratio
            out2 = aug.launch_strong_views([d], [aug.StrongParams(H, W, mic=mask)], chw=False)[0]
            assert np.array_equal(out2.cpu().numpy(), g9[f"mic_{tag}{i}"]), ("mic", tag, i)
            assert out.shape == out2.shape


def test_chw_and_hwc_inputs_give_the_same_bytes():
    from aldi_amd import aug
    augs = _chain(True, (0.5, 32))
    imgs = [_img(H, W, i) for i, (H, W) in enumerate([(211, 333), (800, 1333), (64, 96)])]
    a = aug.strong_views([dev(i.transpose(2, 0, 1)) for i in imgs], augs, chw=True, np_rng=np.random.RandomState(3), py_rng=random.Random(3))
    b = aug.strong_views([dev(i) for i in imgs], augs, chw=False, np_rng=np.random.RandomState(3), py_rng=random.Random(3))
    c = aug.strong_views([dev(i) for i in imgs], augs, chw=False, out_chw=True, np_rng=np.random.RandomState(3), py_rng=random.Random(3))
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy().transpose(2, 0, 1)) and torch.equal(x, z)


def test_batch_of_eight_is_three_calls_and_one_upload(monkeypatch):
    from aldi_amd import _lib as L
    from aldi_amd import aug
    augs = _chain(True, (0.5, 32))
    views = [dev(_img(800, 1333, i).transpose(2, 0, 1)) for i in range(8)]
    calls, uploads = [], []
    real_call, real_upload = L.call, aug._upload
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(aug, "_upload", lambda d, s: (uploads.append(s.numel()), real_upload(d, s))[1])
    for seed in range(4):
        calls.clear(); uploads.clear()
        aug.strong_views(views, augs, np_rng=np.random.RandomState(seed), py_rng=random.Random(seed))
        assert 1 <= len(calls) <= 3 and calls[-1] == "aldi_aug_batch_view", calls
        assert set(calls) <= {"aldi_aug_batch_sums", "aldi_aug_batch_fills", "aldi_aug_batch_view"}
        assert len(uploads) == 1
    torch.cuda.synchronize()


def _cfg(on, contents=("labeled_weak", "labeled_strong", "unlabeled_weak", "unlabeled_strong"), H=96, W=128):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 4, "SYNTHETIC.HEIGHT", H, "SYNTHETIC.WIDTH", W, "SEED", 1, "AUG.DEVICE_STRONG", on,
                         "AUG.UNLABELED_MIC_AUG", True])
    if contents is not None:
        cfg.DATASETS.BATCH_CONTENTS = contents
        cfg.DATASETS.BATCH_RATIOS = tuple(1 for _ in contents)
    return cfg


def test_loader_stage_yields_device_strong_views_of_the_reference_chain():
    from aldi_amd import aug
    from aldi_amd.dataloader import DeviceStrongAugLoader, device_strong_seed
    from aldi_amd.trainer import ALDITrainer
    contents = ("labeled_weak", "labeled_strong", "unlabeled_weak", "unlabeled_strong")
    cfg_on, cfg_off = _cfg(True, contents), _cfg(False, contents)
    on, off = iter(ALDITrainer.build_train_loader(cfg_on)), iter(ALDITrainer.build_train_loader(cfg_off))
    assert isinstance(ALDITrainer.build_train_loader(cfg_on).labeled_loader, DeviceStrongAugLoader)
    rngs = {lab: (np.random.RandomState(device_strong_seed(1, 0, lab)), random.Random(device_strong_seed(1, 0, lab))) for lab in (True, False)}
    np_state = np.random.get_state()[1].copy()
    for step in range(3):
        a, b = next(on), next(off)
        snap = [d["image"].clone() for d in a[1] + a[3]]            # read right after next(), on the current stream, no sync
        assert len(a) == 4 and all(x is not None for x in a)
        for part_on, part_off in zip(a, b):
            assert len(part_on) == len(part_off)
            for d_on, d_off in zip(part_on, part_off):
                assert d_on["image"].is_cuda and d_on["img_weak"].is_cuda
                assert torch.equal(d_on["img_weak"].cpu(), d_off["img_weak"])            # weak views: byte-identical to key off
                assert torch.equal(d_on["instances"]["gt_boxes"], d_off["instances"]["gt_boxes"])
        for k, (part, lab) in enumerate(((a[1], True), (a[3], False))):
            rs, pr = rngs[lab]
            expect = aug.strong_views([d["img_weak"] for d in part], aug.get_strong_augs(cfg_on, lab), np_rng=rs, py_rng=pr)
            for d, e in zip(part, expect):
                assert torch.equal(d["image"], e), (step, lab)
        got = torch.stack([s.flatten()[:4096] for s in snap]).cpu()
        ref = torch.stack([d["image"].flatten()[:4096] for d in a[1] + a[3]]).cpu()
        assert torch.equal(got, ref)
        for d in a[0] + a[2]:                                          # weak parts: image = the weak view
            assert torch.equal(d["image"], d["img_weak"])
    assert np.array_equal(np.random.get_state()[1], np_state)         # global numpy stream untouched


def test_domain_without_strong_view_consumes_no_draws():
    from aldi_amd.dataloader import DeviceStrongAugLoader
    from aldi_amd.trainer import ALDITrainer
    cfg = _cfg(True, ("labeled_weak", "unlabeled_weak"))
    ld = ALDITrainer.build_train_loader(cfg)
    assert isinstance(ld.labeled_loader, DeviceStrongAugLoader) and ld.labeled_loader.augs is None
    it = iter(ld.labeled_loader)
    batch = next(it)
    assert all(torch.equal(d["image"], d["img_weak"]) and d["image"].is_cuda for d in batch)
    from aldi_amd.dataloader import device_strong_seed
    seed = device_strong_seed(1, 0, True)
    fresh = np.random.RandomState(seed)
    assert np.array_equal(it.np_rng.get_state()[1], fresh.get_state()[1]) and it.np_rng.get_state()[2] == fresh.get_state()[2]
    assert it.py_rng.getstate() == random.Random(seed).getstate()


def test_key_off_loader_is_unchanged():
    from aldi_amd.dataloader import SyntheticDetectionLoader, WeakStrongDataloader
    from aldi_amd.trainer import ALDITrainer, _num_classes
    contents = ("labeled_strong", "unlabeled_strong")
    cfg = _cfg(False, contents)
    K = _num_classes(cfg)
    a = iter(ALDITrainer.build_train_loader(cfg))
    b = iter(WeakStrongDataloader(SyntheticDetectionLoader(2, 96, 128, K, 1000, True), SyntheticDetectionLoader(2, 96, 128, K, 2000, False), contents))
    for _ in range(3):
        x, y = next(a), next(b)
        for px, py in zip(x, y):
            assert (px is None) == (py is None)
            for dx, dy in zip(px or [], py or []):
                assert not dx["image"].is_cuda and torch.equal(dx["image"], dy["image"]) and torch.equal(dx["img_weak"], dy["img_weak"])


def test_trainer_runs_graph_replayed_steps_with_the_key_on():
    from aldi_amd.trainer import ALDITrainer
    cfg = _cfg(True, None, H=192, W=256)                              # the reference YAML's own batch contents
    random.seed(4)
    torch.manual_seed(17)
    tr = ALDITrainer(cfg)
    assert tr._trainer.fused
    for it in range(5):
        tr.iter = it
        tr.before_step()
        tr.run_step()
        tr.after_step()
    torch.cuda.synchronize()
    ld = {k: float(v) for k, v in tr._trainer.last_loss_dict.items()}
    assert ld and all(np.isfinite(v) for v in ld.values()), ld
    fs = tr._trainer._fused_step
    assert fs is not None and fs.graph_enabled and fs.stats["replays_a"] >= 1, fs.stats

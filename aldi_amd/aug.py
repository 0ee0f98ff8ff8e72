"""Strong augmentation on the device (reference: aldi/aug.py:39-60 `build_strong_augmentation`, :80-171 transforms).

The reference derives the strong view on the CPU (numpy + scipy's `gaussian_filter`, tens of ms per Cityscapes frame).
Here the weak view lives in HBM as an HWC uint8 tensor and every transform is a HIP kernel (`csrc/aug.hip`); only the
RANDOM DRAWS stay on the host, consumed from the same generators, in the same order, as the reference:

* `np.random.uniform` -- the `RandomApply` gates and the colour weights (detectron2 `Augmentation._rand_range`,
  `RandomContrast/Brightness/Saturation.get_transform`),
* python `random`     -- the blur sigma (drawn inside `RandomBlurTransform.apply_image`, aldi/aug.py:86) and the erase
  geometry (:116-123),
* `np.random.rand`    -- erase fills (:125) and the MIC block mask (:162).

Same class names / constructor arguments as the reference; `apply_image` takes and returns a CUDA uint8 HWC tensor.
"""
from __future__ import annotations

import ctypes
import functools
import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops


def _p(t):
    return t.data_ptr() if t is not None else None


def _check(img: torch.Tensor):
    if not (img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.is_contiguous()):
        raise ValueError("device augmentation expects a contiguous CUDA uint8 HWC image with 3 channels")


# ------------------------------------------------------------------------------------------------ colour (detectron2 names)
class _Blend:
    mode = -1

    def __init__(self, intensity_min: float, intensity_max: float):
        self.intensity_min, self.intensity_max = intensity_min, intensity_max

    def draw(self) -> float:
        return np.random.uniform(self.intensity_min, self.intensity_max)

    def apply_image(self, img: torch.Tensor, w: Optional[float] = None) -> torch.Tensor:
        _check(img)
        if w is None:
            w = self.draw()
        H, W, _ = img.shape
        out = img.clone()
        s = None
        if self.mode == 0:
            s = torch.empty(1, dtype=torch.int64, device=img.device)
            L.call("aldi_aug_sum_u8", _p(out), out.numel(), _p(s), ops.stream_ptr())
        L.call("aldi_aug_blend", _p(out), H, W, self.mode, float(w), _p(s), ops.stream_ptr())
        return out


class RandomContrast(_Blend):
    mode = 0


class RandomBrightness(_Blend):
    mode = 1


class RandomSaturation(_Blend):
    mode = 2


# ------------------------------------------------------------------------------------------------ ALDI-owned transforms
def gaussian_weights(sigma: float, truncate: float = 4.0) -> np.ndarray:
    """the taps scipy's gaussian_filter builds (float64): radius int(truncate * sigma + 0.5)"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


class RandomBlurTransform:
    def __init__(self, sigma: Sequence[float]):
        self.sigma = sigma

    def apply_image(self, img: torch.Tensor, sigma: Optional[float] = None) -> torch.Tensor:
        _check(img)
        if sigma is None:
            sigma = random.uniform(self.sigma[0], self.sigma[1])
        H, W, _ = img.shape
        w = gaussian_weights(sigma)
        wd = torch.from_numpy(w).to(img.device)
        tmp0 = torch.empty(img.numel(), dtype=torch.float32, device=img.device)
        tmp1 = torch.empty_like(tmp0)
        out = torch.empty_like(img)
        L.call("aldi_aug_blur", _p(img), _p(out), _p(tmp0), _p(tmp1), H, W, _p(wd), (len(w) - 1) // 2, ops.stream_ptr())
        return out


class RandomEraseTransform:
    """scale=(sl, sh) of the image area, aspect ratio in (r1, r2), value="random" (uniform noise), as the reference."""
    def __init__(self, sl=0.02, sh=0.4, r1=0.3, r2=3.3, value="random"):
        self.sl, self.sh, self.r1, self.r2, self.value = sl, sh, r1, r2, value

    def draw(self, imgh: int, imgw: int, py_rng=random) -> Optional[Tuple[int, int, int, int]]:
        for _ in range(100):
            area = imgw * imgh
            target_area = py_rng.uniform(self.sl, self.sh) * area
            aspect_ratio = py_rng.uniform(self.r1, self.r2)
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w > 1 and h > 1 and w < imgw and h < imgh:
                h0 = py_rng.randint(0, imgh - h - 1)
                w0 = py_rng.randint(0, imgw - w - 1)
                return h0, w0, h, w
        return None

    def apply_image(self, img: torch.Tensor, rect=None, fill: Optional[np.ndarray] = None) -> torch.Tensor:
        _check(img)
        H, W, C = img.shape
        if rect is None:
            rect = self.draw(H, W)
        if rect is None:
            return img
        h0, w0, h, w = rect
        if fill is None:
            fill = np.random.rand(h, w, C) if self.value == "random" else np.full((h, w, C), float(self.value))
        f32 = torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)).to(img.device)   # the cast the reference's assignment does
        out = img.clone()
        L.call("aldi_aug_erase", _p(out), H, W, h0, w0, h, w, _p(f32), ops.stream_ptr())
        return out


class MICTransform:
    def __init__(self, ratio: float, block_size: int):
        self.ratio, self.block_size = ratio, block_size

    def draw(self, H: int, W: int) -> np.ndarray:
        mh, mw = round(H / self.block_size), round(W / self.block_size)
        return np.random.rand(mh, mw) > self.ratio

    def apply_image(self, img: torch.Tensor, mask: Optional[np.ndarray] = None) -> torch.Tensor:
        _check(img)
        H, W, _ = img.shape
        if mask is None:
            mask = self.draw(H, W)
        m = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to(img.device)
        out = img.clone()
        L.call("aldi_aug_mic", _p(out), H, W, _p(m), int(m.shape[0]), int(m.shape[1]), ops.stream_ptr())
        return out


# ------------------------------------------------------------------------------------------------ the chain
class RandomApply:
    """detectron2 RandomApply: one np.random.uniform draw decides; `aug` is a transform or a list applied in order."""
    def __init__(self, aug, prob: float = 0.5):
        self.aug, self.prob = aug, prob

    def apply_image(self, img: torch.Tensor) -> torch.Tensor:
        if np.random.uniform(0, 1.0) < self.prob:
            for a in (self.aug if isinstance(self.aug, (list, tuple)) else [self.aug]):
                img = a.apply_image(img)
        return img


def build_strong_augmentation(include_erasing: bool = True) -> List[RandomApply]:
    """aldi/aug.py:39-60, same probabilities and ranges"""
    augs = [
        RandomApply([RandomContrast(0.6, 1.4), RandomBrightness(0.6, 1.4), RandomSaturation(0.6, 1.4)], prob=0.8),
        RandomApply(RandomSaturation(0, 0), prob=0.2),                 # random grayscale
        RandomApply(RandomBlurTransform((0.1, 2.0)), prob=0.5),
    ]
    if include_erasing:
        augs += [
            RandomApply(RandomEraseTransform(sl=0.05, sh=0.2, r1=0.3, r2=3.3, value="random"), prob=0.7),
            RandomApply(RandomEraseTransform(sl=0.02, sh=0.2, r1=0.1, r2=6, value="random"), prob=0.5),
            RandomApply(RandomEraseTransform(sl=0.02, sh=0.2, r1=0.05, r2=8, value="random"), prob=0.3),
        ]
    return augs


def get_strong_augs(cfg, labeled: bool) -> List[RandomApply]:
    """the strong part of `get_augs` (aldi/aug.py:26-35): erasing / MIC switches from cfg.AUG"""
    erasing = (labeled and cfg.AUG.LABELED_INCLUDE_RANDOM_ERASING) or (not labeled and cfg.AUG.UNLABELED_INCLUDE_RANDOM_ERASING)
    augs = build_strong_augmentation(include_erasing=erasing)
    if (labeled and cfg.AUG.LABELED_MIC_AUG) or (not labeled and cfg.AUG.UNLABELED_MIC_AUG):
        augs.append(RandomApply(MICTransform(cfg.AUG.MIC_RATIO, cfg.AUG.MIC_BLOCK_SIZE), prob=1.0))
    return augs


def strong_view(img_weak_hwc: torch.Tensor, augs: Sequence[RandomApply], chw: bool = True) -> torch.Tensor:
    """weak view (HWC uint8, device) -> strong view; `chw` returns the (3, H, W) layout dataset dicts carry.  A chain the
    batched kernels run (`recognise_chain`) goes through `strong_views`; anything else through the per-op kernels above.
    Both consume the generators identically and give the same bytes."""
    _check(img_weak_hwc)
    if recognise_chain(augs) is not None:
        return strong_views([img_weak_hwc], augs, chw=False, out_chw=chw)[0]
    img = img_weak_hwc
    for a in augs:
        img = a.apply_image(img)
    if not chw:
        return img
    H, W, _ = img.shape
    out = torch.empty((3, H, W), dtype=torch.uint8, device=img.device)
    L.call("aldi_aug_hwc_to_chw", _p(img), _p(out), H, W, ops.stream_ptr())
    return out



# ------------------------------------------------------------------------------------------------ batched strong views
# N weak views of any sizes -> N strong views in at most three launches (csrc/aug.hip: batch_sums_kernel, fill_kernel,
# view_kernel).  The host only draws: the gates, weights, sigma, rects and MIC mask as `apply_image` would, and for every erase
# fill a snapshot of numpy's MT19937 state every FILL_SEG_WORDS outputs while the state is skipped past the fill
# (aldi_np_mt_advance).  The device replays the fill from those snapshots: the ~0.5 M doubles per 1333x800 view are never
# drawn or copied by the host.
FILL_SEG_WORDS = 624 * 16                     # 32-bit outputs per fill job (16 state refills; even: a job never splits a double)
_HALO = 8                                     # ALDI_AUG_HALO: the largest blur radius of the fused kernel
_COLOUR, _GRAY, _BLUR, _CHW_IN, _CHW_OUT = 1, 2, 4, 8, 16
_TH, _TW, _SUM_CHUNK = 16, 64, 32768


class _AugDesc(ctypes.Structure):
    """aldi_aug_desc (include/aldi_hip.h)"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("sum", ctypes.c_ulonglong),
                ("wc", ctypes.c_double), ("wb", ctypes.c_double), ("ws", ctypes.c_double), ("wg", ctypes.c_double),
                ("taps", ctypes.c_double * (_HALO + 1)), ("fill_off", ctypes.c_long * 3),
                ("H", ctypes.c_int), ("W", ctypes.c_int), ("flags", ctypes.c_int), ("radius", ctypes.c_int),
                ("rect", (ctypes.c_int * 4) * 3), ("nerase", ctypes.c_int), ("mh", ctypes.c_int), ("mw", ctypes.c_int),
                ("tile_begin", ctypes.c_int), ("sum_begin", ctypes.c_int), ("sum_blocks", ctypes.c_int)]


class _FillJob(ctypes.Structure):
    """aldi_aug_fill_job (include/aldi_hip.h)"""
    _fields_ = [("snap", ctypes.c_void_p), ("out_off", ctypes.c_long), ("pos", ctypes.c_int), ("ndoubles", ctypes.c_int)]


class StrongParams:
    """What one image's pass through the chain drew.  colour = (contrast, brightness, saturation) weights or None, gray =
    the grayscale stage's saturation weight or None, sigma = blur sigma or None, erases = [((h0, w0, h, w), snaps [k][624]
    uint32, snap_pos [k] int32)] (snapshot j = numpy's state before output j * FILL_SEG_WORDS of the fill), mic = the bool
    block mask (True = keep) or None."""
    __slots__ = ("H", "W", "colour", "gray", "sigma", "erases", "mic")

    def __init__(self, H: int, W: int, colour=None, gray=None, sigma=None, erases=(), mic=None):
        self.H, self.W, self.colour, self.gray, self.sigma, self.erases, self.mic = H, W, colour, gray, sigma, list(erases), mic

    def ops(self) -> List[tuple]:
        """the oracle's op list (oracle/aug_ops.py draw_strong_params) without the fill arrays: ("erase", rect)"""
        out: List[tuple] = []
        if self.colour is not None:
            out += [("contrast", self.colour[0]), ("brightness", self.colour[1]), ("saturation", self.colour[2])]
        if self.gray is not None:
            out.append(("saturation", self.gray))
        if self.sigma is not None:
            out.append(("blur", self.sigma))
        out += [("erase", rect) for rect, _, _ in self.erases]
        if self.mic is not None:
            out.append(("mic", self.mic))
        return out


def _radius(sigma: float) -> int:
    return int(4.0 * float(sigma) + 0.5)


def recognise_chain(augs) -> Optional[List[tuple]]:
    """[(stage, prob, transforms)] when `augs` is a chain the batched kernels run -- build_strong_augmentation's stages in its
    order, each optional: the colour triple, a lone RandomSaturation (grayscale), a blur whose radius stays within the halo,
    up to three random-value erases, one MIC -- else None (the per-op path takes it)."""
    rank = {"colour": 0, "gray": 1, "blur": 2, "erase": 3, "mic": 4}
    plan, last = [], -1
    for ra in augs:
        if type(ra) is not RandomApply:
            return None
        subs = list(ra.aug) if isinstance(ra.aug, (list, tuple)) else [ra.aug]
        types = tuple(type(a) for a in subs)
        if types == (RandomContrast, RandomBrightness, RandomSaturation):
            kind = "colour"
        elif types == (RandomSaturation,):
            kind = "gray"
        elif types == (RandomBlurTransform,) and 0 < subs[0].sigma[0] <= subs[0].sigma[1] and _radius(subs[0].sigma[1]) <= _HALO:
            kind = "blur"
        elif types == (RandomEraseTransform,) and subs[0].value == "random":
            kind = "erase"
        elif types == (MICTransform,):
            kind = "mic"
        else:
            return None
        if rank[kind] < last or (rank[kind] == last and kind != "erase"):
            return None
        last = rank[kind]
        plan.append((kind, ra.prob, subs))
    if sum(1 for k, _, _ in plan if k == "erase") > 3:
        return None
    return plan


def np_mt_advance(np_rng, n_words: int, seg: int = FILL_SEG_WORDS):
    """Advance numpy's legacy MT19937 (`np.random` or a RandomState) by n_words 32-bit outputs -- what rand(n_words // 2)
    consumes -- without drawing; -> (snaps [k][624] uint32, snap_pos [k] int32), the state before outputs 0, seg, 2 seg, ..."""
    if isinstance(np_rng, np.random.Generator):
        raise TypeError("the strong augmentation replays numpy's legacy MT19937 stream: pass np.random or a RandomState, "
                        "not a numpy Generator")
    st = np_rng.get_state()
    if st[0] != "MT19937":
        raise TypeError(f"unsupported numpy bit generator {st[0]}")
    key = np.array(st[1], dtype=np.uint32)
    pos = ctypes.c_int(int(st[2]))
    nsnap = (n_words + seg - 1) // seg if seg > 0 else 0
    snaps = np.empty((nsnap, 624), dtype=np.uint32)
    snap_pos = np.empty(nsnap, dtype=np.int32)
    L.check(L.lib.aldi_np_mt_advance(key.ctypes.data, ctypes.byref(pos), int(n_words), int(seg), snaps.ctypes.data,
                                     snap_pos.ctypes.data, nsnap), "aldi_np_mt_advance")
    np_rng.set_state((st[0], key, pos.value, st[3], st[4]))
    return snaps, snap_pos


def draw_strong_params(augs, H: int, W: int, np_rng=np.random, py_rng=random) -> StrongParams:
    """Walk the chain for one H x W image, consuming `np_rng` (np.random or a RandomState) and `py_rng` (random or a
    random.Random) in exactly the order and amounts sequential `apply_image` calls do: every gate, the colour weights (the
    grayscale stage's uniform(0, 0) included), sigma, the erase rejection loop (a failed one consumes no fill), each fill
    skipped past with snapshots instead of `rand`, the MIC mask's `rand`."""
    plan = recognise_chain(augs)
    if plan is None:
        raise ValueError("draw_strong_params: not a chain of build_strong_augmentation / get_strong_augs stages")
    if isinstance(np_rng, np.random.Generator):
        raise TypeError("draw_strong_params: pass np.random or a RandomState, not a numpy Generator")
    p = StrongParams(H, W)
    for kind, prob, subs in plan:
        if not np_rng.uniform(0, 1.0) < prob:
            continue
        if kind == "colour":
            p.colour = tuple(float(np_rng.uniform(a.intensity_min, a.intensity_max)) for a in subs)
        elif kind == "gray":
            p.gray = float(np_rng.uniform(subs[0].intensity_min, subs[0].intensity_max))
        elif kind == "blur":
            p.sigma = py_rng.uniform(subs[0].sigma[0], subs[0].sigma[1])
        elif kind == "erase":
            rect = subs[0].draw(H, W, py_rng)
            if rect is not None:
                snaps, snap_pos = np_mt_advance(np_rng, 2 * rect[2] * rect[3] * 3)
                p.erases.append((rect, snaps, snap_pos))
        else:
            m = subs[0]
            p.mic = np_rng.rand(round(H / m.block_size), round(W / m.block_size)) > m.ratio
    return p


def _upload(dst: torch.Tensor, src: torch.Tensor):
    """the batch's one host -> device copy (descriptors, fill jobs, MT snapshots, MIC masks) from pinned memory"""
    dst.copy_(src, non_blocking=True)


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def launch_strong_views(weak_views: Sequence[torch.Tensor], params: Sequence[StrongParams], chw: bool = True,
                        out_chw: Optional[bool] = None) -> List[torch.Tensor]:
    """the device half of `strong_views`: one pinned upload, then at most three launches on the current stream"""
    out_chw = chw if out_chw is None else out_chw
    n = len(weak_views)
    if n == 0:
        return []
    if len(params) != n:
        raise ValueError("launch_strong_views: one StrongParams per view")
    sizes = []
    for v, p in zip(weak_views, params):
        if not (v.is_cuda and v.dtype == torch.uint8 and v.dim() == 3 and v.is_contiguous() and v.shape[0 if chw else 2] == 3):
            raise ValueError(f"strong_views expects contiguous CUDA uint8 {'CHW' if chw else 'HWC'} images with 3 channels")
        H, W = (int(v.shape[1]), int(v.shape[2])) if chw else (int(v.shape[0]), int(v.shape[1]))
        if (H, W) != (p.H, p.W):
            raise ValueError(f"strong_views: parameters drawn for {p.H}x{p.W}, image is {H}x{W}")
        sizes.append((H, W))
    # layout of the upload: [descriptors][fill jobs][snapshots][MIC masks]
    njobs = sum(len(sn) for p in params for _, sn, _ in p.erases)
    off_jobs = _align(n * ctypes.sizeof(_AugDesc))
    off_snaps = _align(off_jobs + njobs * ctypes.sizeof(_FillJob))
    off_masks = _align(off_snaps + njobs * 624 * 4)
    mask_bytes = [0 if p.mic is None else int(np.asarray(p.mic).size) for p in params]
    total = off_masks + sum(mask_bytes)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(total, dtype=torch.uint8, device=weak_views[0].device)
    hbuf, dbase = host.numpy(), dev.data_ptr()
    descs = (_AugDesc * n).from_buffer(hbuf)
    ctypes.memset(ctypes.addressof(descs), 0, off_jobs)
    jobs = (_FillJob * njobs).from_buffer(hbuf, off_jobs) if njobs else None
    snaps = hbuf[off_snaps: off_snaps + njobs * 624 * 4].view(np.uint32).reshape(njobs, 624)
    outs = [torch.empty((3, H, W) if out_chw else (H, W, 3), dtype=torch.uint8, device=v.device) for v, (H, W) in zip(weak_views, sizes)]
    tiles = sum_blocks = arena_bytes = j = 0
    moff = off_masks
    for i, (v, p, (H, W)) in enumerate(zip(weak_views, params, sizes)):
        d = descs[i]
        d.src, d.dst, d.H, d.W = v.data_ptr(), outs[i].data_ptr(), H, W
        d.flags = (_CHW_IN if chw else 0) | (_CHW_OUT if out_chw else 0)
        if p.colour is not None:
            d.flags |= _COLOUR
            d.wc, d.wb, d.ws = (float(w) for w in p.colour)
            d.sum_begin, d.sum_blocks = sum_blocks, (3 * H * W + _SUM_CHUNK - 1) // _SUM_CHUNK
            sum_blocks += d.sum_blocks
        else:
            d.sum_begin = sum_blocks
        if p.gray is not None:
            d.flags |= _GRAY
            d.wg = float(p.gray)
        if p.sigma is not None:
            w = gaussian_weights(p.sigma)
            r = (len(w) - 1) // 2
            if r > _HALO:
                raise ValueError(f"strong_views: blur radius {r} (sigma {p.sigma}) exceeds the fused kernel's halo {_HALO}")
            d.flags |= _BLUR
            d.radius = r
            for k in range(r + 1):
                d.taps[k] = float(w[k])
        if len(p.erases) > 3:
            raise ValueError("strong_views: at most three erase rects per image")
        d.nerase = len(p.erases)
        for e, (rect, sn, sp) in enumerate(p.erases):
            h0, w0, h, w = (int(x) for x in rect)
            if not (h0 >= 0 and w0 >= 0 and h > 0 and w > 0 and h0 + h <= H and w0 + w <= W):
                raise ValueError(f"strong_views: erase rect {rect} outside the {H}x{W} image")
            nd = h * w * 3
            if len(sn) != (2 * nd + FILL_SEG_WORDS - 1) // FILL_SEG_WORDS:
                raise ValueError("strong_views: fill snapshots do not cover the erase rect")
            d.rect[e][0], d.rect[e][1], d.rect[e][2], d.rect[e][3] = h0, w0, h, w
            d.fill_off[e] = arena_bytes
            for k in range(len(sn)):
                jb = jobs[j]
                jb.snap = dbase + off_snaps + j * 624 * 4
                jb.out_off = arena_bytes + k * (FILL_SEG_WORDS // 2)
                jb.pos = int(sp[k])
                jb.ndoubles = min(FILL_SEG_WORDS // 2, nd - k * (FILL_SEG_WORDS // 2))
                j += 1
            snaps[j - len(sn): j] = sn
            arena_bytes += nd
        if p.mic is not None:
            m = np.ascontiguousarray(p.mic, dtype=np.uint8)
            if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
                raise ValueError(f"strong_views: MIC mask of shape {m.shape} for a {H}x{W} image (cv2.resize needs a non-empty mask)")
            d.mh, d.mw = m.shape
            hbuf[moff: moff + m.size] = m.reshape(-1)
            d.mask = dbase + moff
            moff += m.size
        d.tile_begin = tiles
        tiles += ((H + _TH - 1) // _TH) * ((W + _TW - 1) // _TW)
    del descs, jobs                                       # (ctypes views of the pinned buffer)
    arena = torch.empty(max(arena_bytes, 1), dtype=torch.uint8, device=dev.device)
    _upload(dev, host)
    st = ops.stream_ptr()
    if sum_blocks:
        L.call("aldi_aug_batch_sums", dbase, n, sum_blocks, st)
    if njobs:
        L.call("aldi_aug_batch_fills", dbase + off_jobs, njobs, arena.data_ptr(), st)
    L.call("aldi_aug_batch_view", dbase, n, tiles, arena.data_ptr(), st)
    return outs


def strong_views(weak_views: Sequence[torch.Tensor], augs, chw: bool = True, np_rng=np.random, py_rng=random, stream=None,
                 out_chw: Optional[bool] = None, params: Optional[Sequence[StrongParams]] = None) -> List[torch.Tensor]:
    """Batched strong views: `weak_views` are device uint8 images, (3, H, W) when `chw` else (H, W, 3), sizes may differ.
    Draws each image's parameters in order (`draw_strong_params`; or takes `params`), then runs the batch in at most three
    launches on `stream` (default: the current stream).  Outputs are in the input layout unless `out_chw` says otherwise and
    equal, byte for byte, sequential per-op `strong_view` calls consuming the same generators."""
    if params is None:
        params = [draw_strong_params(augs, *((int(v.shape[1]), int(v.shape[2])) if chw else (int(v.shape[0]), int(v.shape[1]))),
                                     np_rng=np_rng, py_rng=py_rng) for v in weak_views]
    if stream is None:
        return launch_strong_views(weak_views, params, chw, out_chw)
    with torch.cuda.stream(stream):
        return launch_strong_views(weak_views, params, chw, out_chw)


# ------------------------------------------------------------------------------------------------ weak views (geometry)
# detectron2's weak chain -- `utils.build_augmentation(cfg, is_train)`: ResizeShortestEdge, then RandomFlip (reference
# aldi/aug.py:16-37) -- on the device (csrc/geom.hip).  As above only the DRAWS and the small tables stay on the host.  The
# resize is Pillow's `Image.resize(BILINEAR)` for uint8 (detectron2 ResizeTransform.apply_image): the coefficient arithmetic
# below is Pillow's precompute_coeffs / normalize_coeffs_8bpc in its operation order and is pinned to Pillow's bytes by
# tests/golden/pil_bilinear.npz.  The detectron2 pieces (output shape, draw order, box transform) restate the published v0.6
# behaviour: PARITY UNPINNED, as oracle/aug_ops.py labels its detectron2 half.
_GEOM_CHW_IN, _GEOM_CHW_OUT, _GEOM_HFLIP, _GEOM_FUSED, _GEOM_VFLIP, _GEOM_SWAP_RB = 1, 2, 4, 8, 16, 32
_GEOM_TH, _GEOM_TW = 16, 64
_PRECISION_BITS = 32 - 8 - 2


class _GeomDesc(ctypes.Structure):
    """aldi_geom_desc (include/aldi_hip.h)"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("tmp", ctypes.c_void_p),
                ("h", ctypes.c_int), ("w", ctypes.c_int), ("new_h", ctypes.c_int), ("new_w", ctypes.c_int), ("flags", ctypes.c_int),
                ("xk_off", ctypes.c_int), ("xb_off", ctypes.c_int), ("xks", ctypes.c_int),
                ("yk_off", ctypes.c_int), ("yb_off", ctypes.c_int), ("yks", ctypes.c_int),
                ("tile_begin", ctypes.c_int), ("h_begin", ctypes.c_int), ("v_begin", ctypes.c_int),
                # the appended tail: the raw image's size and the window's origin; all zero = the window is the whole image
                ("src_h", ctypes.c_int), ("src_w", ctypes.c_int), ("y0", ctypes.c_int), ("x0", ctypes.c_int)]


class ResizeShortestEdge:
    """detectron2 ResizeShortestEdge (parity unpinned): the short side becomes a drawn size, the long side follows and is
    capped at `max_size`.  `get_params` draws from `np_rng` as `get_transform` draws from np.random."""
    def __init__(self, short_edge_length, max_size=2 ** 31 - 1, sample_style="range"):
        if sample_style not in ("range", "choice"):
            raise ValueError(f"ResizeShortestEdge: sample_style {sample_style!r} is neither 'range' nor 'choice'")
        if isinstance(short_edge_length, int):
            short_edge_length = (short_edge_length, short_edge_length)
        short_edge_length = tuple(int(s) for s in short_edge_length)
        if sample_style == "range" and len(short_edge_length) != 2:
            raise ValueError(f"ResizeShortestEdge: short_edge_length must be two values with sample_style 'range', got {short_edge_length}")
        self.short_edge_length, self.max_size, self.sample_style = short_edge_length, max_size, sample_style
        self.is_range = sample_style == "range"

    @staticmethod
    def get_output_shape(oldh: int, oldw: int, short_edge_length: int, max_size: int) -> Tuple[int, int]:
        h, w = oldh, oldw
        size = short_edge_length * 1.0
        scale = size / min(h, w)
        if h < w:
            newh, neww = size, scale * w
        else:
            newh, neww = scale * h, size
        if max(newh, neww) > max_size:
            scale = max_size * 1.0 / max(newh, neww)
            newh, neww = newh * scale, neww * scale
        return int(newh + 0.5), int(neww + 0.5)

    def get_params(self, h: int, w: int, np_rng=np.random) -> Tuple[int, int]:
        if self.is_range:
            size = int(np_rng.randint(self.short_edge_length[0], self.short_edge_length[1] + 1))
        else:
            size = int(np_rng.choice(self.short_edge_length))
        if size == 0:
            return h, w
        return self.get_output_shape(h, w, size, self.max_size)


class RandomFlip:
    """detectron2 RandomFlip (parity unpinned): one uniform(0, 1) draw against `prob`.  A vertical flip is a stage of the full
    chain (`get_view_augs` / `draw_view_params`) only: the device weak view flips horizontally."""
    def __init__(self, prob=0.5, *, horizontal=True, vertical=False):
        if horizontal and vertical:
            raise ValueError("RandomFlip: cannot do both horizontal and vertical")
        if not horizontal and not vertical:
            raise ValueError("RandomFlip: at least one of horizontal or vertical has to be True")
        self.prob, self.horizontal, self.vertical = prob, horizontal, vertical

    def get_params(self, np_rng=np.random) -> bool:
        return bool(np_rng.uniform(0, 1.0) < self.prob)


def get_weak_augs(cfg, is_train: bool) -> list:
    """detectron2 `utils.build_augmentation(cfg, is_train)`: [ResizeShortestEdge] + [RandomFlip] when training and
    INPUT.RANDOM_FLIP is not "none".  What the device path does not run is refused by name."""
    inp = cfg.INPUT
    if inp.get("CROP", {}).get("ENABLED", False):
        raise ValueError("AUG.DEVICE_WEAK: INPUT.CROP.ENABLED is not supported by the device weak view (resize and horizontal flip only)")
    flip = inp.get("RANDOM_FLIP", "horizontal")
    if flip == "vertical":
        raise ValueError('AUG.DEVICE_WEAK: INPUT.RANDOM_FLIP "vertical" is not supported by the device weak view (horizontal or none)')
    if flip not in ("horizontal", "none"):
        raise ValueError(f"AUG.DEVICE_WEAK: unknown INPUT.RANDOM_FLIP {flip!r}")
    if is_train:
        min_size, max_size, style = inp.MIN_SIZE_TRAIN, inp.MAX_SIZE_TRAIN, inp.get("MIN_SIZE_TRAIN_SAMPLING", "choice")
    else:
        min_size, max_size, style = inp.MIN_SIZE_TEST, inp.MAX_SIZE_TEST, "choice"
    augs = [ResizeShortestEdge(min_size if isinstance(min_size, int) else tuple(min_size), max_size, style)]
    if is_train and flip != "none":
        augs.append(RandomFlip(horizontal=True))
    return augs


class WeakParams:
    """what one image's pass through the weak chain drew: (h, w) -> (new_h, new_w), then flipped left-right or not"""
    __slots__ = ("h", "w", "new_h", "new_w", "flip")

    def __init__(self, h: int, w: int, new_h: int, new_w: int, flip: bool = False):
        self.h, self.w, self.new_h, self.new_w, self.flip = int(h), int(w), int(new_h), int(new_w), bool(flip)

    def __eq__(self, other):
        return isinstance(other, WeakParams) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __repr__(self):
        return f"WeakParams({self.h}, {self.w}, {self.new_h}, {self.new_w}, flip={self.flip})"


def draw_weak_params(augs, h: int, w: int, np_rng=np.random) -> WeakParams:
    """consume `np_rng` as detectron2's AugmentationList does for one h x w image: the size draw, then the flip draw"""
    if isinstance(np_rng, np.random.Generator):
        raise TypeError("draw_weak_params: pass np.random or a RandomState, not a numpy Generator")
    new_h, new_w, flip = int(h), int(w), False
    for a in augs:
        if isinstance(a, ResizeShortestEdge):
            new_h, new_w = a.get_params(new_h, new_w, np_rng)
        elif isinstance(a, RandomFlip) and not a.vertical:
            flip ^= a.get_params(np_rng)
        else:
            raise ValueError(f"draw_weak_params: {'a vertical RandomFlip' if isinstance(a, RandomFlip) else type(a).__name__} "
                             "is not a stage of get_weak_augs (the full chain is drawn by draw_view_params)")
    return WeakParams(h, w, new_h, new_w, flip)


@functools.lru_cache(maxsize=256)
def resize_tables(insz: int, outsz: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's bilinear coefficients of one axis insz -> outsz: (k int32 [outsz, ksize] with PRECISION_BITS = 22 fractional
    bits, zero past the tap count; bounds int32 [outsz, 2] = (xmin, tap count)).  ImagingResample's precompute_coeffs +
    normalize_coeffs_8bpc in doubles, in their operation order; the normalising sum runs over the taps left to right."""
    insz, outsz = int(insz), int(outsz)
    if insz < 1 or outsz < 1:
        raise ValueError(f"resize_tables: sizes must be positive, got {insz} -> {outsz}")
    scale = insz / outsz
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(outsz, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), insz)
    n = xmax - xmin
    wts = np.zeros((outsz, ksize), dtype=np.float64)
    ww = np.zeros(outsz, dtype=np.float64)
    for x in range(ksize):
        a = np.abs(((x + xmin).astype(np.float64) - center + 0.5) * ss)
        col = np.where((a < 1.0) & (x < n), 1.0 - a, 0.0)
        wts[:, x] = col
        ww = ww + col                                        # (sequential, as the C loop adds them: np.sum may pair terms)
    nz = ww != 0.0
    wts[nz] = wts[nz] / ww[nz, None]
    k = (0.5 + wts * float(1 << _PRECISION_BITS)).astype(np.int64).astype(np.int32)
    k[np.arange(ksize)[None, :] >= n[:, None]] = 0
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    k.setflags(write=False)
    bounds.setflags(write=False)
    return k, bounds


def _image_layout(img: torch.Tensor, p: WeakParams, chw_in: Optional[bool]) -> bool:
    """True when `img` is (3, h, w), False when (h, w, 3); the parameters' raw size decides, `chw_in` settles a (3, 3, 3) image"""
    if not (img.dtype == torch.uint8 and img.dim() == 3):
        raise ValueError("weak_views expects uint8 images of three dimensions")
    hwc, chw = tuple(img.shape) == (p.h, p.w, 3), tuple(img.shape) == (3, p.h, p.w)
    if chw_in is not None and (chw if chw_in else hwc):
        return bool(chw_in)
    if chw_in is None and (hwc or chw):
        return not hwc
    raise ValueError(f"weak_views: image of shape {tuple(img.shape)} for parameters drawn for {p.h}x{p.w}")


def _launch_geom(images, vparams, layouts, chw_out: bool, outs, who: str) -> List[torch.Tensor]:
    """the one device half of the weak and the windowed views: `vparams` are ViewParams already checked against `images`; one pinned
    upload (descriptors + tables of the WINDOWS' sizes), then one to three launches on the current stream"""
    n = len(images)
    # the tables of the batch, one copy per distinct axis; layout of the upload: [descriptors][tables]
    slots, tabs, nints = {}, [], 1                               # (int 0 is a dummy: `tables` is never an empty buffer)
    for p in vparams:
        for insz, outsz in ((p.w, p.new_w), (p.h, p.new_h)):
            if insz != outsz and (insz, outsz) not in slots:
                k, b = resize_tables(insz, outsz)
                slots[(insz, outsz)] = (nints, nints + k.size, k.shape[1])
                tabs.append((nints, k, b))
                nints += k.size + b.size
    off_tab = _align(n * ctypes.sizeof(_GeomDesc))
    total = off_tab + nints * 4
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    dev = torch.empty(total, dtype=torch.uint8, device=images[0].device)
    hbuf, dbase = host.numpy(), dev.data_ptr()
    descs = (_GeomDesc * n).from_buffer(hbuf)
    ctypes.memset(ctypes.addressof(descs), 0, off_tab)
    tab = hbuf[off_tab:].view(np.int32)
    tab[0] = 0
    for o, k, b in tabs:
        tab[o: o + k.size] = k.reshape(-1)
        tab[o + k.size: o + k.size + b.size] = b.reshape(-1)
    shapes = [(3, p.new_h, p.new_w) if chw_out else (p.new_h, p.new_w, 3) for p in vparams]
    if outs is None:
        outs = [torch.empty(sh, dtype=torch.uint8, device=v.device) for v, sh in zip(images, shapes)]
    else:
        outs = list(outs)
        if len(outs) != n or any(not (o.is_cuda and o.dtype == torch.uint8 and o.is_contiguous() and tuple(o.shape) == sh) for o, sh in zip(outs, shapes)):
            raise ValueError(f"{who}: `outs` must be contiguous CUDA uint8 tensors of shapes {shapes}")
    keep = []                                                    # the two-pass arm's scratch images (stream-ordered: freed after the launches)
    tiles = hblocks = vblocks = 0
    fused = ctypes.c_int(0)
    for i, (v, p, chw) in enumerate(zip(images, vparams, layouts)):
        d = descs[i]
        d.src, d.dst, d.h, d.w, d.new_h, d.new_w = v.data_ptr(), outs[i].data_ptr(), p.h, p.w, p.new_h, p.new_w
        d.flags = ((_GEOM_CHW_IN if chw else 0) | (_GEOM_CHW_OUT if chw_out else 0) | (_GEOM_HFLIP if p.hflip else 0)
                   | (_GEOM_VFLIP if p.vflip else 0) | (_GEOM_SWAP_RB if p.swap_rb else 0))
        if (p.y0, p.x0, p.h, p.w) != (0, 0, p.raw_h, p.raw_w):   # (the tail stays zero for a window that is the whole image)
            d.src_h, d.src_w, d.y0, d.x0 = p.raw_h, p.raw_w, p.y0, p.x0
        if p.w != p.new_w:
            d.xk_off, d.xb_off, d.xks = slots[(p.w, p.new_w)]
        yb = None
        if p.h != p.new_h:
            d.yk_off, d.yb_off, d.yks = slots[(p.h, p.new_h)]
            yb = resize_tables(p.h, p.new_h)[1]
        L.check(L.lib.aldi_geom_plan(yb.ctypes.data if yb is not None else None, p.h, p.new_h, ctypes.byref(fused)), "aldi_geom_plan")
        d.tile_begin, d.h_begin, d.v_begin = tiles, hblocks, vblocks
        if fused.value:
            d.flags |= _GEOM_FUSED
            tiles += ((p.new_h + _GEOM_TH - 1) // _GEOM_TH) * ((p.new_w + _GEOM_TW - 1) // _GEOM_TW)
        else:
            t = torch.empty(p.h * p.new_w * 3, dtype=torch.uint8, device=v.device)
            keep.append(t)
            d.tmp = t.data_ptr()
            hblocks += (p.h * p.new_w + 255) // 256
            vblocks += (p.new_h * p.new_w + 255) // 256
    del descs
    _upload(dev, host)
    L.call("aldi_geom_batch_resize", dbase, n, dbase + off_tab, tiles, hblocks, vblocks, ops.stream_ptr())
    return outs


def launch_weak_views(images: Sequence[torch.Tensor], params: Sequence[WeakParams], chw_out: bool = True,
                      chw_in=None, outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """the device half of `weak_views`: one pinned upload (descriptors + tables), then one to three launches on the current
    stream -- the fused kernel, and the two-pass arm for the images aldi_geom_plan keeps off it.  `outs`: the caller's own
    output tensors (contiguous, of the output shapes) instead of fresh ones.  `chw_in`: None = each image's layout is read off its
    shape and its parameters' raw size; a bool, or one per image, settles it."""
    n = len(images)
    if n == 0:
        return []
    if len(params) != n:
        raise ValueError("launch_weak_views: one WeakParams per image")
    layouts = []
    for v, p, c in zip(images, params, chw_in if isinstance(chw_in, (list, tuple)) else [chw_in] * n):
        layouts.append(_image_layout(v, p, c))
        if not (v.is_cuda and v.is_contiguous()):
            raise ValueError("launch_weak_views expects contiguous CUDA images")
        if min(p.h, p.w, p.new_h, p.new_w) < 1:
            raise ValueError(f"launch_weak_views: empty image in {p}")
    return _launch_geom(images, [ViewParams.whole(p) for p in params], layouts, chw_out, outs, "launch_weak_views")


def weak_views(images: Sequence[torch.Tensor], params: Sequence[WeakParams], chw_out: bool = True, stream=None,
               chw_in=None, outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Batched weak views: `images` are device uint8 images, (h, w, 3) or (3, h, w), sizes may differ; image i is resized to
    params[i]'s (new_h, new_w) as Pillow's BILINEAR resize does, byte for byte, and flipped left-right when params[i].flip.
    Outputs are (3, new_h, new_w) when `chw_out` else (new_h, new_w, 3), on `stream` (default: the current stream)."""
    if stream is None:
        return launch_weak_views(images, params, chw_out, chw_in, outs)
    with torch.cuda.stream(stream):
        return launch_weak_views(images, params, chw_out, chw_in, outs)


def transform_boxes(boxes: np.ndarray, p: WeakParams) -> np.ndarray:
    """detectron2 `transform_instance_annotations` for XYXY boxes under (ResizeTransform, HFlipTransform), float64 (parity
    unpinned): corners scaled by new_w / w and new_h / h, flipped as x -> new_w - x, their min / max, clip(min=0), then the
    minimum with [W, H, W, H]."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    coords = b[:, idxs].reshape(-1, 2).copy()
    coords[:, 0] = coords[:, 0] * (p.new_w * 1.0 / p.w)
    coords[:, 1] = coords[:, 1] * (p.new_h * 1.0 / p.h)
    if p.flip:
        coords[:, 0] = p.new_w - coords[:, 0]
    coords = coords.reshape(-1, 4, 2)
    out = np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1).clip(min=0)
    return np.minimum(out, [p.new_w, p.new_h, p.new_w, p.new_h])


def transform_instances(inst: dict, p) -> dict:
    """the record's instances under the weak view: boxes through `transform_boxes` (a ViewParams: `transform_view_boxes`), cast to
    float32, those with width or height <= 1e-5 -- a box the window cut away, say -- dropped with their classes (detectron2
    filter_empty_instances), image_size = the new size"""
    tfm = transform_boxes if isinstance(p, WeakParams) else transform_view_boxes
    boxes = torch.from_numpy(tfm(inst["gt_boxes"].detach().cpu().numpy(), p)).to(torch.float32)
    keep = ((boxes[:, 2] - boxes[:, 0]) > 1e-5) & ((boxes[:, 3] - boxes[:, 1]) > 1e-5)
    out = dict(inst)
    out["image_size"] = (p.new_h, p.new_w)
    out["gt_boxes"] = boxes[keep]
    for key, val in inst.items():
        if key not in ("gt_boxes", "image_size") and torch.is_tensor(val) and val.dim() >= 1 and val.shape[0] == boxes.shape[0]:
            out[key] = val[keep]
    return out


# ------------------------------------------------------------------------------------------------ the full chain, host half
# detectron2's whole train-time mapper chain for a decoded image -- [RandomCrop] + ResizeShortestEdge + [RandomFlip horizontal |
# vertical] -- as DRAWS and box arithmetic only: what a view with a source window has to be told, and what it does to the boxes.
# Nothing in this block touches the device: `launch_views` at the end of the file is the device half, and
# `launch_weak_views` is the same launch for a window that covers the image.  The two-stage entries above stay as they are.
# The detectron2 pieces restate the published v0.6 behaviour: PARITY UNPINNED.
class RandomCrop:
    """detectron2 RandomCrop (parity unpinned).  `get_params` draws from `np_rng` what `get_transform` draws from np.random, in
    its order: the crop size (relative_range: rand(2); absolute_range: randint for the height, then for the width), then
    randint(h - ch + 1) for y0, then randint(w - cw + 1) for x0."""
    TYPES = ("relative_range", "relative", "absolute", "absolute_range")

    def __init__(self, crop_type: str, crop_size):
        if crop_type not in self.TYPES:
            raise ValueError(f"RandomCrop: crop_type {crop_type!r} is none of {self.TYPES}")
        crop_size = tuple(crop_size)
        if len(crop_size) != 2:
            raise ValueError(f"RandomCrop: crop_size must be two values, got {crop_size}")
        if crop_type == "absolute_range" and not crop_size[0] <= crop_size[1]:
            raise ValueError(f"RandomCrop: absolute_range needs crop_size[0] <= crop_size[1], got {crop_size}")
        self.crop_type, self.crop_size = crop_type, crop_size

    def get_crop_size(self, h: int, w: int, np_rng=np.random) -> Tuple[int, int]:
        if self.crop_type == "relative":
            ch, cw = self.crop_size
            return int(h * ch + 0.5), int(w * cw + 0.5)
        if self.crop_type == "relative_range":
            crop_size = np.asarray(self.crop_size, dtype=np.float32)
            ch, cw = crop_size + np_rng.rand(2) * (1 - crop_size)
            return int(h * ch + 0.5), int(w * cw + 0.5)
        if self.crop_type == "absolute":
            return min(int(self.crop_size[0]), h), min(int(self.crop_size[1]), w)
        ch = int(np_rng.randint(min(h, self.crop_size[0]), min(h, self.crop_size[1]) + 1))
        cw = int(np_rng.randint(min(w, self.crop_size[0]), min(w, self.crop_size[1]) + 1))
        return ch, cw

    def get_params(self, h: int, w: int, np_rng=np.random) -> Tuple[int, int, int, int]:
        """-> (y0, x0, ch, cw)"""
        ch, cw = self.get_crop_size(h, w, np_rng)
        if not (1 <= ch <= h and 1 <= cw <= w):                          # (detectron2 asserts h >= croph and w >= cropw)
            raise ValueError(f"RandomCrop: crop {ch}x{cw} ({self.crop_type} {self.crop_size}) does not fit the {h}x{w} image")
        y0 = int(np_rng.randint(h - ch + 1))
        x0 = int(np_rng.randint(w - cw + 1))
        return y0, x0, ch, cw


def get_view_augs(cfg, is_train: bool) -> list:
    """detectron2's `DatasetMapper.from_config` chain: [RandomCrop] when training and INPUT.CROP.ENABLED, then
    `utils.build_augmentation`: ResizeShortestEdge, and RandomFlip (horizontal or vertical) when training unless INPUT.RANDOM_FLIP
    is "none".  Everything `get_weak_augs` refuses is a stage here."""
    inp = cfg.INPUT
    flip = inp.get("RANDOM_FLIP", "horizontal")
    if flip not in ("horizontal", "vertical", "none"):
        raise ValueError(f"unknown INPUT.RANDOM_FLIP {flip!r}")
    augs = []
    crop = inp.get("CROP", {})
    if is_train and crop.get("ENABLED", False):
        augs.append(RandomCrop(crop.TYPE, crop.SIZE))
    if is_train:
        min_size, max_size, style = inp.MIN_SIZE_TRAIN, inp.MAX_SIZE_TRAIN, inp.get("MIN_SIZE_TRAIN_SAMPLING", "choice")
    else:
        min_size, max_size, style = inp.MIN_SIZE_TEST, inp.MAX_SIZE_TEST, "choice"
    augs.append(ResizeShortestEdge(min_size if isinstance(min_size, int) else tuple(min_size), max_size, style))
    if is_train and flip != "none":
        augs.append(RandomFlip(horizontal=flip == "horizontal", vertical=flip == "vertical"))
    return augs


class ViewParams:
    """what one image's pass through the full chain drew: the window [y0, y0 + h) x [x0, x0 + w) of the raw_h x raw_w image is
    resized to (new_h, new_w), flipped left-right (hflip) and / or upside down (vflip); swap_rb exchanges channels 0 and 2"""
    __slots__ = ("raw_h", "raw_w", "y0", "x0", "h", "w", "new_h", "new_w", "hflip", "vflip", "swap_rb")

    def __init__(self, raw_h: int, raw_w: int, y0: int, x0: int, h: int, w: int, new_h: int, new_w: int, hflip: bool = False,
                 vflip: bool = False, swap_rb: bool = False):
        self.raw_h, self.raw_w, self.y0, self.x0, self.h, self.w = int(raw_h), int(raw_w), int(y0), int(x0), int(h), int(w)
        self.new_h, self.new_w, self.hflip, self.vflip, self.swap_rb = int(new_h), int(new_w), bool(hflip), bool(vflip), bool(swap_rb)

    @classmethod
    def whole(cls, p: WeakParams, swap_rb: bool = False) -> "ViewParams":
        """the two-stage chain's parameters as a window that covers the image"""
        return cls(p.h, p.w, 0, 0, p.h, p.w, p.new_h, p.new_w, hflip=p.flip, swap_rb=swap_rb)

    def __eq__(self, other):
        return isinstance(other, ViewParams) and all(getattr(self, s) == getattr(other, s) for s in self.__slots__)

    def __repr__(self):
        return (f"ViewParams({self.raw_h}, {self.raw_w}, {self.y0}, {self.x0}, {self.h}, {self.w}, {self.new_h}, {self.new_w}, "
                f"hflip={self.hflip}, vflip={self.vflip}, swap_rb={self.swap_rb})")


def draw_view_params(augs, h: int, w: int, np_rng=np.random, swap_rb: bool = False) -> ViewParams:
    """consume `np_rng` as detectron2's AugmentationList does for one h x w image and the chain of `get_view_augs`: the crop
    draws, the size draw for the CROPPED size, the flip draw.  `swap_rb` is not drawn: it is the image's channel order against
    INPUT.FORMAT.  A crop after the resize or the flip is not the mapper's chain and is refused."""
    if isinstance(np_rng, np.random.Generator):
        raise TypeError("draw_view_params: pass np.random or a RandomState, not a numpy Generator")
    y0 = x0 = 0
    ch, cw = int(h), int(w)
    new_h, new_w, hflip, vflip, resized = ch, cw, False, False, False
    for a in augs:
        if isinstance(a, RandomCrop):
            if resized or hflip or vflip or (ch, cw) != (int(h), int(w)):
                raise ValueError("draw_view_params: RandomCrop must be the first stage, once")
            y0, x0, ch, cw = a.get_params(ch, cw, np_rng)
            new_h, new_w = ch, cw
        elif isinstance(a, ResizeShortestEdge):
            new_h, new_w = a.get_params(new_h, new_w, np_rng)
            resized = True
        elif isinstance(a, RandomFlip):
            if a.get_params(np_rng):
                hflip, vflip = hflip ^ a.horizontal, vflip ^ a.vertical
        else:
            raise ValueError(f"draw_view_params: {type(a).__name__} is not a stage of get_view_augs")
    return ViewParams(h, w, y0, x0, ch, cw, new_h, new_w, hflip, vflip, swap_rb)


def transform_view_boxes(boxes: np.ndarray, p: ViewParams) -> np.ndarray:
    """`transform_boxes` under (CropTransform, ResizeTransform, HFlipTransform | VFlipTransform), float64 (parity unpinned):
    corners minus (x0, y0), scaled by new_w / w and new_h / h of the window, x -> new_w - x and / or y -> new_h - y, their
    min / max, clip(min=0), then the minimum with [W, H, W, H]."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    coords = b[:, idxs].reshape(-1, 2).copy()
    coords[:, 0] -= p.x0
    coords[:, 1] -= p.y0
    coords[:, 0] = coords[:, 0] * (p.new_w * 1.0 / p.w)
    coords[:, 1] = coords[:, 1] * (p.new_h * 1.0 / p.h)
    if p.hflip:
        coords[:, 0] = p.new_w - coords[:, 0]
    if p.vflip:
        coords[:, 1] = p.new_h - coords[:, 1]
    coords = coords.reshape(-1, 4, 2)
    out = np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1).clip(min=0)
    return np.minimum(out, [p.new_w, p.new_h, p.new_w, p.new_h])


# ------------------------------------------------------------------------------------------------ the full chain, device half
def _check_window(p: ViewParams, who: str):
    """the window must be a non-empty part of the raw image, the output non-empty: what the kernels would otherwise refuse silently"""
    if min(p.h, p.w, p.new_h, p.new_w, p.raw_h, p.raw_w) < 1:
        raise ValueError(f"{who}: empty window or image in {p}")
    if p.y0 < 0 or p.x0 < 0 or p.y0 + p.h > p.raw_h or p.x0 + p.w > p.raw_w:
        raise ValueError(f"{who}: the window is not inside the {p.raw_h}x{p.raw_w} image in {p}")


def launch_views(images: Sequence[torch.Tensor], params: Sequence[ViewParams], chw_out: bool = True, chw_in=None,
                 outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """the device half of `views`: as `launch_weak_views`, for the full chain.  `images` are the RAW images (raw_h x raw_w, their layout
    read off the shape against the raw size, `chw_in` as there); tables and the choice of the arm follow the WINDOW's sizes; the
    kernels read only the window, flip and exchange R and B at the store.  Everything is checked before the first device call."""
    n = len(images)
    if n == 0:
        return []
    if len(params) != n:
        raise ValueError("launch_views: one ViewParams per image")
    layouts = []
    for v, p, c in zip(images, params, chw_in if isinstance(chw_in, (list, tuple)) else [chw_in] * n):
        if not isinstance(p, ViewParams):
            raise ValueError(f"launch_views: expected a ViewParams, got {type(p).__name__} (ViewParams.whole(p) turns a WeakParams into one)")
        _check_window(p, "launch_views")
        try:
            layouts.append(_image_layout(v, WeakParams(p.raw_h, p.raw_w, p.new_h, p.new_w), c))
        except ValueError as e:
            raise ValueError(str(e).replace("weak_views", "launch_views") + f" (raw size {p.raw_h}x{p.raw_w})") from None
        if not (v.is_cuda and v.is_contiguous()):
            raise ValueError("launch_views expects contiguous CUDA images")
    return _launch_geom(images, list(params), layouts, chw_out, outs, "launch_views")


def views(images: Sequence[torch.Tensor], params: Sequence[ViewParams], chw_out: bool = True, stream=None, chw_in=None,
          outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Batched views of the full mapper chain: image i's window params[i].(y0, x0, h, w) is resized to (new_h, new_w) as Pillow's
    BILINEAR resize of `raw[y0:y0+h, x0:x0+w]` does, byte for byte, then flipped left-right (hflip) and / or upside down (vflip), and
    channels 0 and 2 change places when swap_rb.  Outputs are (3, new_h, new_w) when `chw_out` else (new_h, new_w, 3), on `stream`
    (default: the current stream)."""
    if stream is None:
        return launch_views(images, params, chw_out, chw_in, outs)
    with torch.cuda.stream(stream):
        return launch_views(images, params, chw_out, chw_in, outs)

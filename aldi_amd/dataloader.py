"""The step's input contract (reference aldi/dataloader.py:45-80) plus a synthetic loader.

``unpack_data_weak_strong`` has the reference's semantics: returns
(labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong); weak = deepcopy with
"image" <- "img_weak"; unlabeled_weak is produced whenever ANY unlabeled content is requested."""
import copy
import itertools
import random
import time
from concurrent.futures import ThreadPoolExecutor
from concurrent.futures import TimeoutError as _FutureTimeout

import numpy as np
import torch

from . import synthetic

WEAK_IMG_KEY = "img_weak"


def _weak_view(batch):
    """independent copy of a batch whose "image" is the weakly augmented view (when the mapper attached one)"""
    out = []
    for rec in batch:
        rec = copy.deepcopy(rec)
        weak = rec.get(WEAK_IMG_KEY)
        if weak is not None:
            rec["image"] = weak
        out.append(rec)
    return out


def unpack_data_weak_strong(labeled, unlabeled, batch_contents=("labeled_weak", "labeled_strong", "unlabeled_strong")):
    """-> (labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong), None for what `batch_contents` does not ask for
    (reference aldi/dataloader.py:57-80; pinned by golden g7).  The strong entries are the incoming lists themselves; the weak
    ones are copies.  The unlabeled weak view also exists whenever the strong one is requested: the teacher labels it."""
    wanted = set(batch_contents)
    views = {"labeled": (labeled, {"labeled_weak"}), "unlabeled": (unlabeled, {"unlabeled_weak", "unlabeled_strong"})}
    out = {}
    for prefix, (batch, weak_triggers) in views.items():
        out[prefix + "_weak"] = _weak_view(batch) if batch is not None and wanted & weak_triggers else None
        out[prefix + "_strong"] = batch if prefix + "_strong" in wanted else None
    return out["labeled_weak"], out["labeled_strong"], out["unlabeled_weak"], out["unlabeled_strong"]


class WeakStrongDataloader:
    def __init__(self, labeled_loader, unlabeled_loader, batch_contents=("labeled_weak", "labeled_strong", "unlabeled_strong")):
        self.labeled_loader, self.unlabeled_loader = labeled_loader, unlabeled_loader
        self.batch_contents = batch_contents

    def __iter__(self):
        li = iter(self.labeled_loader) if self.labeled_loader is not None else None
        ui = iter(self.unlabeled_loader) if self.unlabeled_loader is not None else None
        while True:
            yield unpack_data_weak_strong(next(li) if li is not None else None, next(ui) if ui is not None else None,
                                          batch_contents=self.batch_contents)


class SyntheticDetectionLoader:
    """Infinite stream of synthetic COCO-style dicts ({"image": strong view, "img_weak": weak view, "instances"})."""
    def __init__(self, batch_size, h, w, num_classes, seed, labeled: bool, boxes_per_image=(5, 20), fixed: bool = False):
        self.bs, self.h, self.w, self.K, self.seed, self.labeled = batch_size, h, w, num_classes, seed, labeled
        self.boxes_per_image, self.fixed = boxes_per_image, fixed

    def __iter__(self):
        it = 0
        while True:
            g = torch.Generator().manual_seed(self.seed + (0 if self.fixed else it))
            batch = []
            for _ in range(self.bs):
                nb = int(torch.randint(self.boxes_per_image[0], self.boxes_per_image[1] + 1, (1,), generator=g))
                img, inst = synthetic.make_image(self.h, self.w, nb, self.K, g)
                if not self.labeled:
                    inst = {"image_size": (self.h, self.w), "gt_boxes": torch.zeros(0, 4), "gt_classes": torch.zeros(0, dtype=torch.int64)}
                batch.append({"image": synthetic.strong_view(img, g), WEAK_IMG_KEY: img, "instances": inst})
            it += 1
            yield batch


def device_strong_seed(base: int, rank: int, labeled: bool) -> int:
    """the private draw seed of one rank's labeled / unlabeled DeviceStrongAugLoader (`base` = cfg.SEED, or 0 when unset)"""
    return (base * 1000003 + (3000 if labeled else 4000) + 17 * rank) % 2 ** 32


def device_weak_seed(base: int, rank: int, labeled: bool) -> int:
    """the private seed of one rank's labeled / unlabeled WEAK draws (size, flip): a third stream, apart from the strong ones"""
    return (base * 1000003 + (5000 if labeled else 6000) + 17 * rank) % 2 ** 32


RAW_IMG_KEY = "image_raw"


class DeviceStrongAugLoader:
    """Wraps a loader that yields lists of dicts carrying `img_weak` (uint8 CHW, host or device) and builds every strong view on
    the device (aldi_amd/aug.py `strong_views`: the reference's chain, three launches per batch).  Each yielded dict is a
    shallow copy with `img_weak` = the device weak view and `image` = its strong view (`augs` None: the weak view itself, and
    nothing is drawn).

    The draws come from a private RandomState / random.Random seeded with `seed` (as detectron2 seeds each loader worker),
    so the process's global streams are never touched.  It runs one batch ahead: batch k+1's host work (the inner loader,
    the draws) on a background thread, its copies and launches on a side stream, while the caller runs step k; `next()`
    only makes the caller's current stream wait for the batch (no host sync).

    `weak` (aldi_amd/aug.py `get_weak_augs`; default None = everything above, unchanged) adds the weak view's geometry to the
    SAME stage: the record's decoded image -- `image_raw`, uint8 (H, W, 3) or (3, H, W), host or device; absent: `img_weak` --
    is resized and flipped on the device (`launch_weak_views`) into `img_weak`, (3, new_h, new_w), on the same side stream
    and ahead of the strong launches, which then work on it.  The size and flip draws come from a third private RandomState
    seeded with `weak_seed`; `instances` are transformed on the host (`transform_instances`), `height` / `width` keep the
    raw size.  The background thread still does host work only: every launch is issued by the caller's thread.

    `weak` may also be the FULL mapper chain (aldi_amd/aug.py `get_view_augs`: [RandomCrop] + ResizeShortestEdge + RandomFlip horizontal
    or vertical).  `view` says which: None (default) recognises the full chain by a RandomCrop member or a vertical RandomFlip -- a
    list of `get_weak_augs` never has either, so it keeps the path above draw for draw; True forces the full-chain path (the
    file-backed loaders do, so that `swap_rb` works without a crop); False refuses nothing and keeps the two-stage path.  On the full-chain
    path the draws are `draw_view_params(weak, h, w, weak_rng, swap_rb=swap_rb)`, the launch is `launch_views` on the RAW image (crop,
    both flips and the R <-> B exchange of `swap_rb` inside the kernels), and `instances` go through the same `transform_instances`."""

    def __init__(self, loader, augs, seed: int, device=None, weak=None, weak_seed=None, view=None, swap_rb: bool = False):
        self.loader, self.augs, self.seed, self.device = loader, augs, int(seed), device
        self.weak, self.weak_seed = weak, int(seed if weak_seed is None else weak_seed)
        if view is None:
            from . import aug
            view = weak is not None and any(isinstance(a, aug.RandomCrop) or (isinstance(a, aug.RandomFlip) and a.vertical) for a in weak)
        self.view, self.swap_rb = bool(view), bool(swap_rb)
        if (self.view or self.swap_rb) and weak is None:
            raise ValueError("DeviceStrongAugLoader: `view` / `swap_rb` need the chain in `weak`")
        if self.swap_rb and not self.view:
            raise ValueError("DeviceStrongAugLoader: `swap_rb` is done by the full-chain view: pass view=True")

    def __iter__(self):
        return _DeviceStrongAugIter(self)


class _DeviceStrongAugIter:
    def __init__(self, owner: DeviceStrongAugLoader):
        self.it = iter(owner.loader)
        self.augs = owner.augs
        self.np_rng, self.py_rng = np.random.RandomState(owner.seed), random.Random(owner.seed)
        self.weak, self.view, self.swap_rb = owner.weak, owner.view, owner.swap_rb
        self.weak_rng = np.random.RandomState(owner.weak_seed) if owner.weak is not None else None
        self.device = torch.device(owner.device) if owner.device is not None else torch.device("cuda", torch.cuda.current_device())
        self.side = torch.cuda.Stream(self.device)
        self.pool = ThreadPoolExecutor(1)
        self.ready = self.future = None
        self.done = False

    def _prepare(self):
        """host work (background thread): the inner loader's batch, pinned weak views, the draws in image order"""
        from . import aug
        batch = next(self.it)
        if self.weak is not None:
            return self._prepare_weak(batch)
        weak, params = [], []
        for rec in batch:
            w = rec[WEAK_IMG_KEY]
            if w.dtype != torch.uint8 or w.dim() != 3 or w.shape[0] != 3:
                raise ValueError(f"DeviceStrongAugLoader: `{WEAK_IMG_KEY}` must be a uint8 (3, H, W) image")
            weak.append(w.contiguous() if w.is_cuda else w.contiguous().pin_memory())
            if self.augs is not None:
                params.append(aug.draw_strong_params(self.augs, int(w.shape[1]), int(w.shape[2]), np_rng=self.np_rng, py_rng=self.py_rng))
        return batch, weak, params

    def _prepare_weak(self, batch):
        """host work with the weak stage on: the size / flip draws, the (cached) resize tables, the pinned raw images, the
        transformed instances, then the strong draws for the NEW sizes"""
        from . import aug
        raws, wparams, params, out = [], [], [], []
        for rec in batch:
            raw = rec.get(RAW_IMG_KEY, rec.get(WEAK_IMG_KEY))
            if raw is None or raw.dtype != torch.uint8 or raw.dim() != 3 or 3 not in (raw.shape[0], raw.shape[2]):
                raise ValueError(f"DeviceStrongAugLoader: `{RAW_IMG_KEY}` (or `{WEAK_IMG_KEY}`) must be a uint8 (H, W, 3) or (3, H, W) image")
            chw = RAW_IMG_KEY not in rec or raw.shape[2] != 3          # (`img_weak` is CHW by contract; an (H, W, 3) raw image is HWC)
            h, w = (int(raw.shape[1]), int(raw.shape[2])) if chw else (int(raw.shape[0]), int(raw.shape[1]))
            if self.view:
                wp = aug.draw_view_params(self.weak, h, w, self.weak_rng, swap_rb=self.swap_rb)
            else:
                wp = aug.draw_weak_params(self.weak, h, w, self.weak_rng)
            for insz, outsz in ((wp.w, wp.new_w), (wp.h, wp.new_h)):
                if insz != outsz:
                    aug.resize_tables(insz, outsz)
            raws.append((raw.contiguous() if raw.is_cuda else raw.contiguous().pin_memory(), chw))
            wparams.append(wp)
            rec = dict(rec)
            rec.pop(RAW_IMG_KEY, None)
            if rec.get("instances") is not None:
                rec["instances"] = aug.transform_instances(rec["instances"], wp)
            rec.setdefault("height", h)
            rec.setdefault("width", w)
            out.append(rec)
            if self.augs is not None:
                params.append(aug.draw_strong_params(self.augs, wp.new_h, wp.new_w, np_rng=self.np_rng, py_rng=self.py_rng))
        return out, (raws, wparams), params

    def _issue(self, prepared):
        """device work (caller's thread): weak-view copies and the batch's launches on the side stream"""
        from . import aug
        batch, weak, params = prepared
        raws = None
        if self.weak is not None:
            raws, wparams = weak
            weak = [r for r, _ in raws]
        if any(w.is_cuda for w in weak):
            self.side.wait_stream(torch.cuda.current_stream(self.device))       # device weak views come from the caller's stream
        with torch.cuda.device(self.device), torch.cuda.stream(self.side):
            dweak = [w if w.is_cuda else w.to(self.device, non_blocking=True) for w in weak]
            if raws is not None:                                                # H2D copy -> resize + flip -> (below) the strong launches
                draw = dweak
                dweak = (aug.launch_views if self.view else aug.launch_weak_views)(draw, wparams, chw_out=True, chw_in=[chw for _, chw in raws])
                for t, (r, _) in zip(draw, raws):
                    if r.is_cuda:                                               # a caller's device image: the side stream is its last user
                        t.record_stream(self.side)
            strong = aug.launch_strong_views(dweak, params, chw=True) if self.augs is not None else dweak
            ev = torch.cuda.Event()
            ev.record(self.side)
        out = []
        for rec, w, s in zip(batch, dweak, strong):
            rec = dict(rec)
            rec[WEAK_IMG_KEY], rec["image"] = w, s
            out.append(rec)
        return out, ev, [t for t in dweak + list(strong) if t.device.type == "cuda"]

    def _submit(self):
        self.future = self.pool.submit(self._prepare)

    def __iter__(self):
        return self

    def __next__(self):
        if self.done:
            raise StopIteration
        if self.ready is None:
            self.ready = self._issue(self._prepare())
            self._submit()
        out, ev, tensors = self.ready
        try:
            self.ready = self._issue(self.future.result())
            self._submit()
        except StopIteration:
            self.done = True
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in tensors:
            t.record_stream(cur)                        # the caching allocator must not hand them out before the caller is done
        return out

    def __del__(self):
        pool = getattr(self, "pool", None)
        if pool is not None:
            pool.shutdown(wait=False)


# ------------------------------------------------------------------------------------------------ file-backed loaders
# Rules that keep this from hanging: no worker processes (decode parallelism is a ThreadPoolExecutor sized from DATALOADER.NUM_WORKERS,
# at most MAX_DECODE_THREADS); no device call from a decode thread (the mapper builds numpy arrays and CPU tensors only); work is
# demand-driven and finite (`next()` submits one batch of decode futures plus at most one batch of look-ahead: no producer loop, no
# bounded queue, so a dropped iterator leaves no thread blocked); every wait has a limit; a training stream never ends.
MAX_DECODE_THREADS = 16
DECODE_TIMEOUT_S = 120.0                      # per batch: generous for sixteen 2048 x 1024 PNGs on one slow disk, short of "forever"


def file_sampler_seed(base: int, labeled: bool) -> int:
    """the seed of the labeled / unlabeled TrainingSampler's permutations (`base` = cfg.SEED, or 0 when unset).  Every rank uses the SAME
    seed -- the rank enters through the stride `[rank::world]` of the shared stream, which is what keeps the ranks' shards disjoint --
    and it is a fourth stream, apart from the strong and weak draw seeds above."""
    return (base * 1000003 + (7000 if labeled else 8000)) % 2 ** 32


class TrainingSampler:
    """detectron2's: an infinite stream of indices.  One torch.Generator seeded once yields a fresh `randperm(size)` per epoch
    (`arange(size)` without `shuffle`); rank r of `world` takes elements r, r + world, ... of the concatenated stream."""
    def __init__(self, size: int, shuffle: bool = True, seed: int = 0, rank: int = 0, world: int = 1):
        if not isinstance(size, int) or size <= 0:
            raise ValueError(f"TrainingSampler: size must be a positive integer, got {size!r}")
        if not 0 <= rank < world:
            raise ValueError(f"TrainingSampler: rank {rank} is not in [0, {world})")
        self.size, self.shuffle, self.seed, self.rank, self.world = size, bool(shuffle), int(seed), int(rank), int(world)

    def _infinite_indices(self):
        g = torch.Generator()
        g.manual_seed(self.seed)
        while True:
            yield from (torch.randperm(self.size, generator=g) if self.shuffle else torch.arange(self.size)).tolist()

    def __iter__(self):
        return itertools.islice(self._infinite_indices(), self.rank, None, self.world)


class InferenceSampler:
    """detectron2's: rank r of `world` gets one contiguous shard of range(size); the first size % world shards are one longer"""
    def __init__(self, size: int, rank: int = 0, world: int = 1):
        if not isinstance(size, int) or size < 0:
            raise ValueError(f"InferenceSampler: size must be a non-negative integer, got {size!r}")
        if not 0 <= rank < world:
            raise ValueError(f"InferenceSampler: rank {rank} is not in [0, {world})")
        shard, left = divmod(size, world)
        sizes = [shard + int(r < left) for r in range(world)]
        begin = sum(sizes[:rank])
        self.indices = range(begin, min(begin + sizes[rank], size))

    def __iter__(self):
        return iter(self.indices)

    def __len__(self):
        return len(self.indices)


class FileDetectionLoader:
    """Lists of `batch_size` mapped records of `dataset_dicts` in the sampler's order, decoded by `num_threads` threads (at most
    MAX_DECODE_THREADS).  With a TrainingSampler the stream never ends (a dataset smaller than a batch simply wraps) and never raises
    StopIteration; with an InferenceSampler it is finite, has `__len__`, and its last batch may be short.  `timeout`: seconds one batch
    may take to decode (DECODE_TIMEOUT_S); past it `next()` raises a TimeoutError that names the file it was waiting for.  An exception on
    a decode thread is raised by `next()` with the file's name.  `close()` cancels what has not started and shuts the pool."""

    def __init__(self, dataset_dicts, mapper, batch_size: int, sampler, num_threads: int = 4, timeout: float = DECODE_TIMEOUT_S):
        if batch_size < 1:
            raise ValueError(f"FileDetectionLoader: batch_size must be positive, got {batch_size}")
        if not len(dataset_dicts):
            raise ValueError("FileDetectionLoader: no records")
        self.dataset_dicts, self.mapper, self.batch_size, self.sampler = dataset_dicts, mapper, int(batch_size), sampler
        self.num_threads = max(1, min(MAX_DECODE_THREADS, int(num_threads)))
        self.timeout = float(timeout)
        self._pool = None

    def _executor(self) -> ThreadPoolExecutor:
        if self._pool is None:
            self._pool = ThreadPoolExecutor(self.num_threads, thread_name_prefix="aldi-decode")
        return self._pool

    def __len__(self):
        if not hasattr(self.sampler, "__len__"):
            raise TypeError("FileDetectionLoader: a training stream has no length")
        return (len(self.sampler) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        return _FileIter(self)

    def close(self):
        pool, self._pool = getattr(self, "_pool", None), None
        if pool is not None:
            pool.shutdown(wait=False, cancel_futures=True)             # (no wait without a limit: a running decode is finite and its
                                                                       #  thread ends with it; the interpreter joins the threads at exit)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FileIter:
    def __init__(self, owner: FileDetectionLoader):
        self.owner = owner
        self.indices = iter(owner.sampler)
        self.endless = not hasattr(owner.sampler, "__len__")
        self.pending = None                                            # the look-ahead: at most one batch of futures
        self.started = False

    def _submit_batch(self):
        idx = list(itertools.islice(self.indices, self.owner.batch_size))
        if not idx:
            return None
        pool, dicts, mapper = self.owner._executor(), self.owner.dataset_dicts, self.owner.mapper
        return [(str(dicts[i].get("file_name", i)), pool.submit(mapper, dicts[i])) for i in idx]

    def __iter__(self):
        return self

    def __next__(self):
        if not self.started:
            self.started, self.pending = True, self._submit_batch()
        cur = self.pending
        if cur is None:
            if self.endless:
                raise RuntimeError("FileDetectionLoader: the training sampler ran out of indices; a training stream must not end")
            raise StopIteration
        self.pending = self._submit_batch()
        deadline = time.monotonic() + self.owner.timeout
        out = []
        for k, (name, fut) in enumerate(cur):
            try:
                out.append(fut.result(timeout=max(0.0, deadline - time.monotonic())))
            except BaseException as e:
                for _, f in cur[k + 1:]:
                    f.cancel()
                if isinstance(e, _FutureTimeout) and not fut.done():
                    raise TimeoutError(f"FileDetectionLoader: decoding {name} did not finish within the batch's {self.owner.timeout:g} s") from None
                if not isinstance(e, Exception):
                    raise
                if isinstance(e, StopIteration) or name not in str(e):     # (a StopIteration from a record must not end the stream)
                    raise RuntimeError(f"FileDetectionLoader: decoding {name} failed: {type(e).__name__}: {e}") from e
                raise
        return out


class DeviceTestViewLoader:
    """The test-time view over a finite FileDetectionLoader: each record's decoded image is uploaded and resized on the device by the
    chain of `get_view_augs(cfg, False)` (ResizeShortestEdge at MIN_SIZE_TEST / MAX_SIZE_TEST, nothing drawn; `swap_rb` for
    INPUT.FORMAT) when its batch is asked for -- lazily, on the caller's thread and current stream.  Yields lists of {image: device
    uint8 CHW, image_id, height, width, file_name}; `height` / `width` stay the RAW size, so the evaluators' rescaling brings the
    detections back."""

    def __init__(self, loader: FileDetectionLoader, augs, swap_rb: bool = False, device=None):
        self.loader, self.augs, self.swap_rb, self.device = loader, augs, bool(swap_rb), device

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        from . import aug
        device = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        rng = np.random.RandomState(0)                                 # (the test chain draws nothing: one size, no flip)
        for batch in self.loader:
            raws = [rec["image_raw"].to(device) for rec in batch]
            params = [aug.draw_view_params(self.augs, int(r.shape[0]), int(r.shape[1]), rng, swap_rb=self.swap_rb) for r in raws]
            imgs = aug.launch_views(raws, params, chw_out=True, chw_in=False)
            yield [{"image": im, "image_id": rec["image_id"], "height": rec["height"], "width": rec["width"], "file_name": rec["file_name"]}
                   for im, rec in zip(imgs, batch)]

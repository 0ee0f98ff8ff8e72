"""ALDITrainer and the step drivers behind the reference's names (aldi/trainer.py:28-246,
aldi/dropin.py:29-184).  The iteration's schedule -- source weak/strong, target-weak alignment,
distillation, loss-key suffixes, 1/accum scaling -- is a table (``plan_micro_steps``) executed either
chunk by chunk (``run_model_labeled_unlabeled``, the reference's order) or as one fused student pass
(``fused_step.FusedStep``; ``fused_run_model_detr`` for the Deformable-DETR detector) on the HIP engine."""
from __future__ import annotations

import contextlib
import copy
import logging
import os
import time
import weakref
from typing import Callable, Dict, List, NamedTuple, Optional

from collections import OrderedDict

import torch
import torch.distributed as dist

from . import synthetic
from .dataloader import DeviceStrongAugLoader, SyntheticDetectionLoader, WeakStrongDataloader, device_strong_seed, device_weak_seed
from .distill import build_distiller
from .ema import EMA
from .model import build_aldi

DEBUG = False
debug_dict = {}


class MicroStep(NamedTuple):
    """One row of the iteration's schedule: which batch goes through the student (or through the distiller together with
    the teacher's batch), with which forward flags, under which loss-key suffix, and which of its losses count."""
    name: str                                   # loss-key suffix
    data: Optional[list]                        # student inputs
    teacher_data: Optional[list]                # set => the distiller runs this row (teacher inputs = weak views)
    kwargs: dict                                # forward flags of model(...)
    keep: Callable[[str], bool]                 # losses that contribute (the others are multiplied by 0 / not reported)


def plan_micro_steps(labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong, *, do_align: bool, do_distill: bool) -> List[MicroStep]:
    """The schedule of one Mean-Teacher iteration as data (contract: reference aldi/trainer.py:28-117):
    labeled weak and strong views are plain supervised rows that keep every loss; with alignment on the unlabeled weak
    views go through the student only for their "_da_" losses; with distillation on the distiller sees (weak, strong)
    pairs and keeps everything it names.  Both drivers below -- the sequential one and the fused one -- execute this plan."""
    everything = lambda k: True
    plan: List[MicroStep] = []
    if labeled_weak is not None:
        plan.append(MicroStep("source_weak", labeled_weak, None, {"do_align": do_align}, everything))
    if labeled_strong is not None:
        plan.append(MicroStep("source_strong", labeled_strong, None, {"do_align": do_align}, everything))
    if do_align:
        plan.append(MicroStep("target_weak", unlabeled_weak, None, {"labeled": False, "do_align": True}, lambda k: "_da_" in k))
    if do_distill:
        plan.append(MicroStep("distill", unlabeled_strong, unlabeled_weak, {}, lambda k: k != "_"))
    return plan


def _schedule_flags(trainer):
    core = getattr(trainer.model, "module", trainer.model)
    do_align = any(getattr(core, a, None) is not None for a in ("img_align", "ins_align"))
    return do_align, trainer.distiller.distill_enabled()


def run_model_labeled_unlabeled(trainer, labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong):
    """Sequential driver of the plan (the reference's schedule, aldi/trainer.py:28-117): IMS_PER_GPU-sized chunks one after
    the other, each followed by its own backward unless BACKWARD_AT_END; every reported loss is divided by the number of
    gradient-accumulation steps = (|labeled_weak| + |labeled_strong| + |unlabeled_weak|) // IMS_PER_GPU (unlabeled_strong is
    not counted).  Returns {f"{loss}_{suffix}": 0-d tensor} (detached when the backward already ran)."""
    do_align, do_distill = _schedule_flags(trainer)
    plan = plan_micro_steps(labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong, do_align=do_align, do_distill=do_distill)
    bs = trainer.model_batch_size
    accum = sum(len(part or []) for part in (labeled_weak, labeled_strong, unlabeled_weak)) // bs
    early = not trainer.backward_at_end
    if DEBUG:
        debug_dict.update(last_labeled_weak=copy.deepcopy(labeled_weak), last_labeled_strong=copy.deepcopy(labeled_strong),
                          last_unlabeled_weak=copy.deepcopy(unlabeled_weak), last_unlabeled_strong=copy.deepcopy(unlabeled_strong))
    metrics: Dict[str, torch.Tensor] = {}
    # head statistics (SOLVER.LOG_PERIOD): the engine counts beside its loss kernels for the micro-step named here (those that report the
    # detection losses); chunks of one micro-step add their counts and their images
    sink = getattr(getattr(getattr(trainer.model, "module", trainer.model), "engine", None), "stats_sink", None)
    if sink is not None:
        sink.set_images({})
    for row in plan:
        if row.teacher_data is not None:
            assert len(row.teacher_data) == len(row.data), "Teacher and student data must be the same length."
        for lo in range(0, len(row.data), bs):
            chunk = row.data[lo:lo + bs]
            if sink is not None and row.keep("loss_cls"):
                sink.current = row.name
                sink.add_images(row.name, len(chunk))
            try:
                if row.teacher_data is not None:
                    losses = trainer.distiller(row.teacher_data[lo:lo + bs], chunk)
                else:
                    losses = trainer.model(chunk, **row.kwargs)
            finally:
                if sink is not None:
                    sink.current = None
            if early:               # non-contributing losses still enter the graph with weight 0 (every parameter gets a gradient)
                trainer.do_backward(sum(v if row.keep(k) else v * 0 for k, v in losses.items()) / accum, override=True)
            for k, v in losses.items():
                if row.keep(k):
                    key = f"{k}_{row.name}"
                    v = v / accum
                    metrics[key] = metrics.get(key, 0) + (v.detach() if early else v)
    if DEBUG and do_distill:
        debug_dict["last_pseudolabeled"] = copy.deepcopy(unlabeled_strong)
    return metrics


def fused_run_model_detr(trainer, labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong):
    """the plan of `run_model_labeled_unlabeled` for the Deformable-DETR detector with its student passes FUSED (reference schedule:
    aldi/trainer.py:28-117 with HardDistiller, aldi/distill.py:62-84): the teacher pseudo-labels every target chunk first (the EMA tick of
    this iteration has run; the teacher does not depend on the student's passes), then all student chunks -- source and pseudo-labelled
    target -- go through ONE trunk + transformer pass and ONE backward (`DeformableDETR.forward_fused`: the set criterion per chunk, so
    matching, normalisers, loss keys, the 1 / accum scaling and the early-backward semantics are the sequential driver's)."""
    model = trainer.model
    do_align, do_distill = _schedule_flags(trainer)
    plan = plan_micro_steps(labeled_weak, labeled_strong, unlabeled_weak, unlabeled_strong, do_align=do_align, do_distill=do_distill)
    bs = trainer.model_batch_size
    accum = sum(len(part or []) for part in (labeled_weak, labeled_strong, unlabeled_weak)) // bs
    parts, rows, pairs = [], [], []
    for row in plan:
        for lo in range(0, len(row.data), bs):
            chunk = row.data[lo:lo + bs]
            if row.teacher_data is not None:
                pairs.append((row.teacher_data[lo:lo + bs], chunk))
            parts.append(chunk)
            rows.append(row)
    # the teacher's inference (what HardDistiller.__call__ runs before the student's pass) on the second stream, beside the student's label-free
    # forward: its pseudo labels are first read by the set criterion
    side = _teacher_stream(model.device) if pairs else None
    main = torch.cuda.current_stream()
    if side is not None:
        side.wait_stream(main)
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for weak, strong in pairs:
            trainer.distiller.pseudo_labeler(weak, strong)
    ctx = model.forward_fused_begin(parts)
    if side is not None:
        main.wait_stream(side)
    ctx, losses = model.forward_fused_finish(ctx, parts)
    model.backward_fused(ctx, [1.0 / accum] * len(parts))
    trainer._detr_fused_steps = getattr(trainer, "_detr_fused_steps", 0) + 1
    metrics: Dict[str, torch.Tensor] = {}
    for row, ld in zip(rows, losses):
        for k, v in ld.items():
            if row.keep(k):
                key = f"{k}_{row.name}"
                metrics[key] = metrics.get(key, 0) + (v / accum).detach()
    if DEBUG and do_distill:
        debug_dict["last_pseudolabeled"] = copy.deepcopy(unlabeled_strong)
    return metrics


def _data_parallel() -> bool:
    """more than one rank -- or ALDI_DP_FORCE=1 with an initialised process group of any size: the data-parallel code path (bucketed
    exchange, its stream plumbing, the captured collectives) on a single GPU, which is how the RCCL path is exercised on a 1-GPU box"""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size() > 1 or os.environ.get("ALDI_DP_FORCE", "0") == "1"


_TEACHER_STREAMS = {}


def _teacher_stream(device):
    """second HIP stream for the teacher's inference (ALDI_TEACHER_STREAM=0 keeps everything on one stream)"""
    if os.environ.get("ALDI_TEACHER_STREAM", "1") != "1" or torch.device(device).type != "cuda":
        return None
    key = str(device)
    if key not in _TEACHER_STREAMS:
        # (ALDI_TEACHER_PRIO: HIP stream priority of the teacher's branch, e.g. -1 = above the student's; measured)
        _TEACHER_STREAMS[key] = torch.cuda.Stream(device=device, priority=int(os.environ.get("ALDI_TEACHER_PRIO", "0")))
    return _TEACHER_STREAMS[key]


def _num_classes(cfg) -> int:
    """the detector's class count: ROI_HEADS.NUM_CLASSES, or DEFORMABLE_DETR.NUM_CLASSES for that meta-architecture"""
    if cfg.MODEL.META_ARCHITECTURE == "DeformableDETR":
        return int(cfg.MODEL.DEFORMABLE_DETR.NUM_CLASSES)
    return int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)


def clip_spec_from_cfg(cfg):
    """SOLVER.CLIP_GRADIENTS -> None (no node, or ENABLED False) | ops.ClipSpec.  detectron2's maybe_add_gradient_clipping knows
    CLIP_TYPE value | norm (per parameter tensor); full_model is the DETR wrapper's one global norm.  Values the kernels do not
    implement are rejected, never ignored (the rule of D2Params.from_cfg)."""
    from .ops import ClipSpec
    node = cfg.SOLVER.get("CLIP_GRADIENTS", None)
    if node is None or not node.get("ENABLED", False):
        return None
    clip_type = node.get("CLIP_TYPE", "value")
    if clip_type not in ("value", "norm", "full_model"):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE must be one of value, norm, full_model, got {node.get('CLIP_TYPE')!r}")
    raw = node.get("NORM_TYPE", 2.0)
    try:
        norm_type = float(raw)
    except (TypeError, ValueError):
        norm_type = None
    if norm_type not in (2.0, float("inf")):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE must be 2.0 or inf, got {raw!r}")
    raw = node.get("CLIP_VALUE", 1.0)
    try:
        clip_value = float(raw)
    except (TypeError, ValueError):
        clip_value = float("nan")
    if not (0.0 < clip_value < float("inf")):
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_VALUE must be a positive finite number, got {raw!r}")
    return ClipSpec(clip_type, clip_value, norm_type)


class EngineSGD:
    """torch.optim.SGD-shaped handle on the fused HIP optimizer (momentum / weight decay of detectron2's build_optimizer)."""
    def __init__(self, model, lr, momentum=0.9, weight_decay=1e-4, clip=None):
        """clip: None | ops.ClipSpec (SOLVER.CLIP_GRADIENTS, `clip_spec_from_cfg`): shown in param_groups[0]["clip"], not checkpoint state"""
        self.model = model
        self.param_groups = [{"lr": lr, "momentum": momentum, "weight_decay": weight_decay}]
        if clip is not None:
            self.param_groups[0]["clip"] = clip

    @property
    def clip(self):
        return self.param_groups[0].get("clip")

    def zero_grad(self, set_to_none: bool = False):
        self.model.weights.zero_grad()

    def step(self):
        W = self.model.weights
        if getattr(W, "_sgd_applied", False):        # the fused step ran this iteration's update inside its backward (FusedStep.run(sgd=...))
            W._sgd_applied = False
            W._after_sgd()
            return
        g = self.param_groups[0]
        if self.clip is None:
            W.sgd_step(g["lr"], g["momentum"], g["weight_decay"])
        else:
            W.sgd_step(g["lr"], g["momentum"], g["weight_decay"], clip=self.clip)

    def state_dict(self):
        """checkpointable (detectron2 saves the optimizer through `trainer._trainer.optimizer`): the flat momentum buffer"""
        W = self.model.weights
        return {"format": "aldi_amd.flat_sgd", "param_groups": [{k: v for k, v in g.items() if k != "clip"} for g in self.param_groups],
                "momentum_buffer": None if W._mom is None else W.mom.detach().cpu().clone(), "first_step": bool(W.first_step)}

    def load_state_dict(self, sd):
        W = self.model.weights
        if sd.get("format") != "aldi_amd.flat_sgd":
            logging.getLogger(__name__).warning("optimizer state of a foreign format: momentum restarts from zero")
            return
        for g, h in zip(self.param_groups, sd.get("param_groups", [])):
            g.update({k: v for k, v in h.items() if k in ("momentum", "weight_decay")})
        if sd.get("momentum_buffer") is not None:
            W.mom.copy_(sd["momentum_buffer"].to(W.mom.device))
        W.first_step = bool(sd.get("first_step", sd.get("momentum_buffer") is None))


class EngineAdamW:
    """torch.optim.AdamW-shaped handle on the fused HIP AdamW of the ViTDet / ConvNeXt models (reference aldi/backbone.py:66-84:
    detectron2 common/optim.py AdamW -- betas (0.9, 0.999), weight_decay 0.1, none on the norms and on pos_embed).
    `lr_decay_rate` = ViTDet's layer-wise lr decay, which the reference turns on exactly for build_vitdet_b_backbone
    (aldi/trainer.py:204 -> get_vit_lr_decay_rate(num_layers=12, lr_decay_rate=0.7))."""
    def __init__(self, model, lr, weight_decay=0.1, betas=(0.9, 0.999), lr_decay_rate=None, num_layers=12):
        self.model = model
        self.param_groups = [{"lr": lr, "weight_decay": weight_decay, "betas": betas}]
        self.lr_decay_rate, self.num_layers = lr_decay_rate, num_layers

    def zero_grad(self, set_to_none: bool = False):
        self.model.weights.zero_grad()

    def step(self):
        g = self.param_groups[0]
        kw = {}
        if self.lr_decay_rate is not None:
            kw = dict(lr_decay_rate=self.lr_decay_rate, num_layers=self.num_layers)
        self.model.weights.adamw_step(g["lr"], betas=g["betas"], weight_decay=g["weight_decay"], **kw)

    def state_dict(self):
        W = self.model.weights
        has = getattr(W, "_m", None) is not None
        return {"format": "aldi_amd.flat_adamw", "param_groups": [dict(g) for g in self.param_groups], "step": int(getattr(W, "step_count", 0)),
                "exp_avg": W._m.detach().cpu().clone() if has else None, "exp_avg_sq": W._v.detach().cpu().clone() if has else None}

    def load_state_dict(self, sd):
        W = self.model.weights
        if sd.get("format") != "aldi_amd.flat_adamw":
            logging.getLogger(__name__).warning("optimizer state of a foreign format: AdamW moments restart from zero")
            return
        if sd.get("exp_avg") is not None:
            W._m = sd["exp_avg"].to(W.device).clone()
            W._v = sd["exp_avg_sq"].to(W.device).clone()
        W.step_count = int(sd.get("step", 0))


class EngineDetrAdamW:
    """AdamW of the Deformable-DETR detector over its flat state: the parameter groups and the full-model gradient clip of
    configs/Base-DETR.yaml:59-69 (DetrWeights.adamw_step)"""
    def __init__(self, model, cfg):
        S = cfg.SOLVER
        self.model = model
        self.param_groups = [{"lr": S.BASE_LR, "weight_decay": S.WEIGHT_DECAY, "betas": (0.9, 0.999)}]
        cg = S.CLIP_GRADIENTS
        self.clip = float(cg.CLIP_VALUE) if cg.ENABLED else 0.0
        if cg.ENABLED and (cg.CLIP_TYPE != "full_model" or float(cg.NORM_TYPE) != 2.0):
            raise ValueError("DeformableDETR: only CLIP_TYPE full_model with the L2 norm is implemented")
        self.backbone_mult, self.proj_mult, self.proj_names = float(S.BACKBONE_LR_MULTIPLIER), float(S.LR_LINEAR_PROJ_MULTIPLIER), tuple(S.LR_LINEAR_PROJ_NAMES)

    def zero_grad(self, set_to_none: bool = False):
        self.model.weights.zero_grad()

    def step(self):
        g = self.param_groups[0]
        self.model.weights.adamw_step(g["lr"], betas=g["betas"], weight_decay=g["weight_decay"], clip=self.clip, backbone_mult=self.backbone_mult,
                                      proj_mult=self.proj_mult, proj_names=self.proj_names)

    def state_dict(self):
        W = self.model.weights
        return {"format": "aldi_amd.detr_adamw", "param_groups": [dict(g) for g in self.param_groups], "step": int(W.step),
                "exp_avg": None if W.m is None else W.m.detach().cpu().clone(), "exp_avg_sq": None if W.v is None else W.v.detach().cpu().clone()}

    def load_state_dict(self, sd):
        W = self.model.weights
        if sd.get("format") != "aldi_amd.detr_adamw":
            logging.getLogger(__name__).warning("optimizer state of a foreign format: the Deformable-DETR AdamW moments restart from zero")
            return
        if sd.get("exp_avg") is not None:
            W.m, W.v = sd["exp_avg"].to(W.master.device).clone(), sd["exp_avg_sq"].to(W.master.device).clone()
        W.step = int(sd.get("step", 0))


class WarmupMultiStepLR:
    """detectron2 WarmupMultiStepLR (linear warmup), stepped once per iteration."""
    def __init__(self, optimizer, base_lr, steps, gamma, warmup_factor, warmup_iters):
        self.opt, self.base_lr, self.steps, self.gamma = optimizer, base_lr, tuple(steps), gamma
        self.warmup_factor, self.warmup_iters = warmup_factor, warmup_iters
        self.last_iter = 0
        self._apply()

    def lr_at(self, it):
        wf = 1.0
        if it < self.warmup_iters:
            alpha = it / self.warmup_iters
            wf = self.warmup_factor * (1 - alpha) + alpha
        return self.base_lr * wf * self.gamma ** sum(1 for s in self.steps if s <= it)

    def _apply(self):
        self.opt.param_groups[0]["lr"] = self.lr_at(self.last_iter)

    def step(self):
        self.last_iter += 1
        self._apply()

    def state_dict(self):
        return {"last_epoch": self.last_iter}           # torch's scheduler key name

    def load_state_dict(self, sd):
        self.last_iter = int(sd["last_epoch"])
        self._apply()


class SimpleTrainer:
    """One iteration = fetch, zero_grad, run_model, backward, (all-reduce), optimizer step (aldi/dropin.py:87-130)."""
    iter = 0                                         # set by the owning trainer before every run_step (detectron2: self._trainer.iter)
    metric_recorder = None                           # events.DeviceMetricRecorder when SOLVER.LOG_PERIOD > 0 (DefaultTrainer._setup_metrics)

    def __init__(self, model, data_loader, optimizer, zero_grad_before_forward=False):
        self.model, self.data_loader, self.optimizer = model, data_loader, optimizer
        self._data_loader_iter_obj = None
        self.zero_grad_before_forward = zero_grad_before_forward
        self.last_loss_dict: Dict[str, float] = {}

    @property
    def _data_loader_iter(self):
        if self._data_loader_iter_obj is None:
            self._data_loader_iter_obj = iter(self.data_loader)
        return self._data_loader_iter_obj

    def run_step(self):
        """One optimizer step = fetch a batch, run the model (which may already contain its backward), reduce gradients across ranks,
        apply the update.  Same order of effects as the reference's step (aldi/dropin.py:94-121), organised around what THIS engine
        can take over: `run_model` may clear the gradients itself, run the backward itself (`_fused_done`) and even the update."""
        if not self.model.training:
            raise AssertionError("[SimpleTrainer] model was changed to eval mode!")
        t0 = time.perf_counter()
        batch = self._fetch_batch()
        fetch_s = time.perf_counter() - t0
        clear_first = self.zero_grad_before_forward
        if clear_first and self._defers_zero_grad():
            self._zero_pending = True                # the fused step clears them on a side stream beside its forward
        elif clear_first:
            self.optimizer.zero_grad()
        if self._defers_sgd():
            self._sgd_pending = True                 # the fused step may apply this iteration's update inside its backward
        result = self.run_model(batch)
        self.__dict__.pop("_sgd_pending", None)
        fused = bool(getattr(self, "_fused_done", False))
        if isinstance(result, torch.Tensor):
            loss_dict, total = {"total_loss": result}, result
        else:
            # (a fused step has nothing left to differentiate; summing its entries would only put a dozen tiny launches before the update)
            loss_dict, total = result, (None if fused else sum(result.values()))
        if not clear_first and not fused:
            self.optimizer.zero_grad()
        self.do_backward(total)
        self.after_backward()
        self._write_metrics(loss_dict, fetch_s)
        self.optimizer.step()

    def run_model(self, data):
        return self.model(data)

    def _wants_lookahead(self) -> bool:
        """True when run_model can use batch k + 1 while it runs step k (the fused step's cross-step pipelining of the frozen prefix)"""
        return False

    def _fetch_batch(self):
        """the batch of this step; with look-ahead the NEXT one is fetched too (the reference's loader is asynchronous and always a batch ahead,
        aldi/trainer.py:211-238, aldi/dataloader.py:45-55) and left in `_next_batch` for run_model -- the order of batches is unchanged"""
        if not self._wants_lookahead():
            ahead = self.__dict__.pop("_ahead_batch", None)
            self._next_batch = None
            return ahead if ahead is not None else next(self._data_loader_iter)
        ahead = self.__dict__.pop("_ahead_batch", None)
        batch = ahead if ahead is not None else next(self._data_loader_iter)
        try:
            self._ahead_batch = next(self._data_loader_iter)
        except StopIteration:
            self._ahead_batch = None
        self._next_batch = self._ahead_batch
        return batch

    def _defers_zero_grad(self) -> bool:
        """True when run_model clears the gradients itself (the fused step does it on a side stream beside its forward)"""
        return False

    def _defers_sgd(self) -> bool:
        """True when run_model may run this iteration's optimizer step itself (and then sets weights._sgd_applied for EngineSGD.step)"""
        return False

    def do_backward(self, losses):
        losses.backward()

    def after_backward(self):
        """One all-reduce of the student gradients per step (the reference's DDP reduces on every
        micro-step backward, aldi/dropin.py:53; the sum is linear so one reduction at the end is equivalent)."""
        if _data_parallel():
            red = getattr(self, "_reducer", None)
            if red is not None:                  # fused step: most of the exchange already ran under the backward
                red.finish()
                self._reducer = None
            else:
                dist.all_reduce(self.model.weights.grad, op=dist.ReduceOp.SUM)
            self.model.weights.scale_grad(1.0 / dist.get_world_size())

    def _write_metrics(self, loss_dict, data_time):
        """the reference reads every loss with .item() here (a host wait per step); with a recorder the values go into its device ring by
        one launch on the current stream -- the step's last loss is final, no graph is being captured -- and reach the host at the flush"""
        self.last_loss_dict = loss_dict
        self.last_data_time = data_time
        if self.metric_recorder is not None:
            self.metric_recorder.record(loss_dict, None, self.iter, data_time=data_time)


class AMPTrainer(SimpleTrainer):
    """Reference: fp16 autocast + GradScaler (aldi/dropin.py:131-184).  Here AMP means the bf16 compute mode of the
    engine (fp32 master weights / accumulators); bf16 needs no loss scaling, so there is no GradScaler."""
    def run_step(self):
        assert self.model.training, "[AMPTrainer] model was changed to eval mode!"
        assert torch.cuda.is_available(), "[AMPTrainer] CUDA is required for AMP training!"
        super().run_step()


class _ALDITrainer:
    def __init__(self, model, data_loader, optimizer, distiller, backward_at_end=True, model_batch_size=None):
        super().__init__(model, data_loader, optimizer, zero_grad_before_forward=not backward_at_end)
        self.distiller = distiller
        self.backward_at_end = backward_at_end
        self.model_batch_size = model_batch_size
        self.fused = False

    def _fusable_distiller(self) -> bool:
        """the fused driver evaluates ALDIDistiller's losses with its own kernels and does not fire the models' hook points: it stands in
        only for the built-in distiller -- the class itself, or a subclass that overrides none of the loss / forward methods -- and only
        while nobody else listens on the student's or the teacher's hook points (a third-party distiller or a user's SaveIO tap would be
        silently bypassed: those take the reference's sequential schedule, logged once)"""
        from .distill import ALDIDistiller
        from .helpers import foreign_hooks
        d = self.distiller
        why = None
        if not isinstance(d, ALDIDistiller):
            why = "distiller %s is not ALDIDistiller" % type(d).__name__
        elif any(getattr(type(d), m) is not getattr(ALDIDistiller, m) for m in ("__call__", "_distill_forward", "get_rpn_losses", "get_roih_losses", "register_hooks")):
            why = "distiller %s overrides a loss / forward method of ALDIDistiller" % type(d).__name__
        else:
            own = [getattr(d, a) for side in d._TAPS.values() for a, _ in side] + [d.seeder, d.teacher_proposal_replacer]
            models = [m.module if hasattr(m, "module") else m for m in (d.student, d.teacher)]
            if any(foreign_hooks(m, own) for m in models):
                why = "a forward (pre-)hook that the distiller did not register sits on the student or the teacher"
        if why is not None and not self.__dict__.get("_fuse_warned"):
            self._fuse_warned = True
            import logging
            logging.getLogger(__name__).warning("fused step not used (%s): taking the reference's sequential schedule", why)
        return why is None

    def _can_fuse(self, data):
        """the fused driver (`fused_step.FusedStep`, the only one for the R-CNN engines) takes the reference's FPN batch contents (labeled_strong [+ unlabeled weak / strong pairs]) in any whole
        number of IMS_PER_GPU-sized micro-batches per part -- e.g. the shipped IMS_PER_BATCH 48 / IMS_PER_GPU 2 on 8 GPUs = three
        source and three distillation micro-steps (reference configs/Base-RCNN-FPN.yaml:15-16, aldi/trainer.py:51-52) -- as long as
        the whole iteration fits one student pass (16 images: the staging kernels' limit)"""
        lw, ls, uw, us = data
        bs = self.model_batch_size
        from .engine import RCNN
        if not isinstance(getattr(self.model, "engine", None), RCNN):        # (e.g. the Deformable-DETR detector: sequential driver)
            return False
        if not self.fused or lw is not None or ls is None or len(ls) == 0 or len(ls) % bs or hasattr(self.model, "module"):
            return False
        do_align, do_distill = _schedule_flags(self)
        total = len(ls)
        if do_distill:
            if not self._fusable_distiller() or uw is None or us is None:
                return False
            if len(uw) != len(us) or len(us) == 0 or len(us) % bs:
                return False
            total += len(us)
        if do_align:
            if uw is None or len(uw) == 0 or len(uw) % bs:
                return False
            total += len(uw)
        if total > 16:
            return False
        return True

    def _can_fuse_detr(self, data) -> bool:
        """the Deformable-DETR detector's fused student pass (fused_run_model_detr): plain source + hard-pseudo-label batches with an early
        backward per chunk (every loss kept with the weight 1 / accum), the built-in HardDistiller (or none), nobody listening on the hook
        points, and chunks that share ONE padded canvas -- the input projections' GroupNorm runs over the canvas, so a chunk padded to a
        larger one than its own would normalise differently than `model(chunk)` does"""
        lw, ls, uw, us = data
        bs = self.model_batch_size
        model = self.model
        if not getattr(model, "detr", False) or not self.fused or hasattr(model, "module") or self.backward_at_end:
            return False
        if lw is not None or ls is None or len(ls) == 0 or len(ls) % bs:
            return False
        do_align, do_distill = _schedule_flags(self)
        if do_align:
            return False
        chunks = [ls[i:i + bs] for i in range(0, len(ls), bs)]
        if do_distill:
            from .distill import HardDistiller
            from .helpers import foreign_hooks
            d = self.distiller
            if type(d) is not HardDistiller or uw is None or us is None or len(uw) != len(us) or len(us) == 0 or len(us) % bs:
                return False
            if any(foreign_hooks(m.module if hasattr(m, "module") else m, []) for m in (d.student, d.teacher)):
                return False
            chunks += [us[i:i + bs] for i in range(0, len(us), bs)]
        if sum(len(c_) for c_ in chunks) > 16:
            return False
        canvas = {(max(int(b["image"].shape[-2]) for b in c_), max(int(b["image"].shape[-1]) for b in c_)) for c_ in chunks}
        return len({((h + 31) // 32, (w + 31) // 32) for h, w in canvas}) == 1

    def _wants_lookahead(self) -> bool:
        from .engine import RCNN
        from .fused_step import pipeline_prefix_requested
        model = self.model.module if hasattr(self.model, "module") else self.model
        eng = getattr(model, "engine", None)
        return (bool(self.fused) and pipeline_prefix_requested(model.cfg)
                and type(eng) is RCNN and eng.prefix_pipelinable())

    def _defers_zero_grad(self) -> bool:
        from .engine import RCNN
        model = self.model.module if hasattr(self.model, "module") else self.model
        # (only the flat R50 weight container: the ViTDet / ConvNeXt models keep their trunk's gradients in a second buffer)
        return bool(self.fused) and type(getattr(model, "engine", None)) is RCNN

    def _defers_sgd(self) -> bool:
        W = getattr(self.model, "weights", None)
        # (never while the optimizer clips: a full_model norm needs every gradient before the first update, and the per-layer-group
        #  launches inside the backward know no coefficient -- the same rule for all three clip types)
        return (self._defers_zero_grad() and isinstance(self.optimizer, EngineSGD) and self.optimizer.clip is None and not _data_parallel()
                and W is not None and not W.first_step and os.environ.get("ALDI_SGD_IN_STEP", "0") == "1")

    def run_model(self, data):
        self._fused_done = False
        pending_ema = self.__dict__.pop("_pending_ema", None)       # the EMA tick `before_step` left for the fused step to run
        if pending_ema is not None and not self._can_fuse(data):
            pending_ema[0].update_weights(self.model, pending_ema[1])
            pending_ema = None
        defer = self.__dict__.pop("_zero_pending", False)          # run_step left the zero_grad of this iteration to this method
        if defer and not self._can_fuse(data):
            self.optimizer.zero_grad()               # (this batch takes the unfused path)
            defer = False
        if self._can_fuse(data):
            self._fused_done = True
            if not self.zero_grad_before_forward:    # the fused driver runs its backward inside run_model
                if self._defers_zero_grad():
                    defer = True
                else:
                    self.optimizer.zero_grad()
            eng = self.model.engine
            reducer = None
            if _data_parallel():
                from .reduce import BucketedReducer, resolve_exchange
                reducer = self._reducer = BucketedReducer(self.model.weights.grad, payload=str(self.model.cfg.SOLVER.get("GRAD_PAYLOAD", "fp32")),
                                                          exchange=resolve_exchange(self.model.cfg.SOLVER.get("GRAD_EXCHANGE", "auto")))
                eng.grad_ready = reducer.ready
            ok = False
            try:
                if getattr(self, "_fused_step", None) is None:
                    from .fused_step import FusedStep
                    self._fused_step = FusedStep(self)
                sgd = None
                if self.__dict__.pop("_sgd_pending", False) and reducer is None:
                    g_ = self.optimizer.param_groups[0]
                    sgd = (g_["lr"], g_["momentum"], g_["weight_decay"])
                out = self._fused_step.run(*data, ema=pending_ema, zero_grad=defer, reducer=reducer, sgd=sgd,
                                           next_data=self.__dict__.get("_next_batch") if self._wants_lookahead() else None)
                ok = True
                return out
            finally:
                eng.grad_ready = None
                if not ok:
                    self._reducer = None         # a failed step must not leave its half-used reducer to the next `after_backward`
        if self._can_fuse_detr(data):
            self._fused_done = True
            return fused_run_model_detr(self, *data)
        return run_model_labeled_unlabeled(self, *data)

    def do_backward(self, losses, override=False):
        if getattr(self, "_fused_done", False):
            return                                   # the fused driver already ran its single backward
        if self.backward_at_end or override:
            super().do_backward(losses)


class ALDIAMPTrainer(_ALDITrainer, AMPTrainer):
    pass


class ALDISimpleTrainer(_ALDITrainer, SimpleTrainer):
    pass


class DefaultTrainer:
    """Constructor sequence of the reference's DefaultTrainer (aldi/dropin.py:35-70) without the Detectron2 hook zoo."""
    metric_recorder = None                           # events.DeviceMetricRecorder when SOLVER.LOG_PERIOD > 0 (_setup_metrics)

    def __init__(self, cfg):
        self.cfg = cfg
        model = self.build_model(cfg)
        optimizer = self.build_optimizer(cfg, model)
        data_loader = self.build_train_loader(cfg)
        model = self.create_ddp_model(model, broadcast_buffers=False, cfg=cfg)
        self._trainer = self._create_trainer(cfg, model, data_loader, optimizer)
        self.scheduler = self.build_lr_scheduler(cfg, optimizer)
        self.checkpointer = self._create_checkpointer(model, cfg)
        self.start_iter = 0
        self.iter = 0
        self.max_iter = cfg.SOLVER.MAX_ITER
        self._setup_metrics(cfg)

    def _create_trainer(self, cfg, model, data_loader, optimizer):
        return (AMPTrainer if cfg.SOLVER.AMP.ENABLED else SimpleTrainer)(model, data_loader, optimizer)

    def _setup_metrics(self, cfg):
        """SOLVER.LOG_PERIOD > 0: the device recorder (every rank: its flush is collective under data parallelism), the event storage and --
        main process only -- the console and metrics.json writers; the R-CNN engine gets the recorder's sink BEFORE the first step, so that
        the step graphs are captured with the statistics launches.  0: nothing is created, the step is launched exactly as without this."""
        period = int(cfg.SOLVER.get("LOG_PERIOD", 0) or 0)
        if period <= 0:
            return
        from .events import CommonMetricPrinter, DeviceMetricRecorder, EventStorage, JSONWriter
        model = self._trainer.model
        core = getattr(model, "module", model)
        device = torch.device(getattr(core, "device", None) or cfg.MODEL.DEVICE)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        rec = DeviceMetricRecorder(period, device, max_iter=self.max_iter)
        rec.storage = self.storage = EventStorage(self.start_iter)
        if self._is_main_process():
            rec.writers.append(CommonMetricPrinter(self.max_iter))
            if cfg.OUTPUT_DIR:
                rec.writers.append(JSONWriter(os.path.join(cfg.OUTPUT_DIR, "metrics.json")))
        self.metric_recorder = self._trainer.metric_recorder = rec
        eng = getattr(core, "engine", None)
        if eng is not None and hasattr(type(eng), "stats_sink"):
            eng.stats_sink = rec.sink

    def flush_metrics(self):
        """the open logging window -> storage and writers; raises FloatingPointError when a recorded loss was not finite.  Called every
        LOG_PERIOD iterations, after the last one, and as the first statement of everything that persists or judges state."""
        if self.metric_recorder is not None:
            self.metric_recorder.flush()

    def create_ddp_model(self, model, broadcast_buffers, cfg):
        """One process per GPU; gradients are all-reduced over RCCL in SimpleTrainer.after_backward.  Rank 0's weights are broadcast once."""
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.broadcast(model.weights.master, src=0)
            model.weights.refresh()
        return model

    @classmethod
    def build_lr_scheduler(cls, cfg, optimizer):
        S = cfg.SOLVER
        return WarmupMultiStepLR(optimizer, S.BASE_LR, S.STEPS, S.GAMMA, S.WARMUP_FACTOR, S.WARMUP_ITERS)

    @classmethod
    def build_optimizer(cls, cfg, model):
        clip = clip_spec_from_cfg(cfg)
        if clip is None:
            return EngineSGD(model, cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM, cfg.SOLVER.WEIGHT_DECAY)
        return EngineSGD(model, cfg.SOLVER.BASE_LR, cfg.SOLVER.MOMENTUM, cfg.SOLVER.WEIGHT_DECAY, clip=clip)

    def _create_checkpointer(self, model, cfg, ckpt_cls=None):
        """aldi/dropin.py:77-82: the trainer itself (iteration, LR-scheduler hook, optimizer) is a checkpointable"""
        from .checkpoint import DetectionCheckpointer
        return (ckpt_cls or DetectionCheckpointer)(model, cfg.OUTPUT_DIR, trainer=weakref.proxy(self))

    def state_dict(self):
        """detectron2 TrainerBase / SimpleTrainer.state_dict layout"""
        ret = {"iteration": self.iter, "hooks": {"LRScheduler": self.scheduler.state_dict()}}
        opt = self._trainer.optimizer
        if hasattr(opt, "state_dict"):
            ret["_trainer"] = {"optimizer": opt.state_dict()}
        return ret

    def load_state_dict(self, sd):
        self.iter = int(sd["iteration"])
        sched = sd.get("hooks", {}).get("LRScheduler")
        if sched is not None:
            self.scheduler.load_state_dict(sched)
        else:                                            # file without scheduler state: the schedule is a function of the iteration
            self.scheduler.load_state_dict({"last_epoch": self.iter + 1})
        opt = sd.get("_trainer", {}).get("optimizer")
        if opt is not None and hasattr(self._trainer.optimizer, "load_state_dict"):
            self._trainer.optimizer.load_state_dict(opt)

    def resume_or_load(self, resume=True):
        """detectron2 DefaultTrainer.resume_or_load: last checkpoint of OUTPUT_DIR when resuming (model, EMA, optimizer momentum,
        LR schedule position and iteration continue), else cfg.MODEL.WEIGHTS (an empty string = keep the initial weights)."""
        ret = self.checkpointer.resume_or_load(self.cfg.MODEL.WEIGHTS, resume=resume)
        if resume and self.checkpointer.has_checkpoint():
            if "trainer" not in ret:                     # e.g. a file written by an evaluation-only tool
                self.iter = int(ret.get("iteration", -1))
                self.scheduler.load_state_dict({"last_epoch": self.iter + 1})
            self.start_iter = self.iter + 1
            self.iter = self.start_iter
        return ret

    @property
    def model(self):
        return self._trainer.model

    def before_step(self):
        pass

    def run_step(self):
        self._trainer.iter = self.iter
        self._trainer.run_step()

    def _is_main_process(self):
        return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0

    def after_step(self):
        """LRScheduler hook, then detectron2's PeriodicCheckpointer (fvcore): `model_{iter:07d}` every SOLVER.CHECKPOINT_PERIOD
        iterations and `model_final` after the last one, main process only."""
        rec = self.metric_recorder
        if rec is not None:
            now = time.perf_counter()
            rec.note_step(time_s=now - self.__dict__.get("_t_after_step", now), lr=float(self._trainer.optimizer.param_groups[0]["lr"]))
            self._t_after_step = now
        self.scheduler.step()
        period = int(self.cfg.SOLVER.get("CHECKPOINT_PERIOD", 0) or 0)
        last = self.iter >= self.max_iter - 1
        save_now = period > 0 and (self.iter + 1) % period == 0 and not last
        if rec is not None and ((self.iter + 1) % rec.period == 0 or last or save_now):
            self.flush_metrics()                     # (every rank; before any checkpoint: a non-finite loss raises here, nothing is saved from it)
        if self._is_main_process() and self.cfg.OUTPUT_DIR:
            if save_now:
                self.checkpointer.save("model_{:07d}".format(self.iter), iteration=self.iter)
            if last:
                self.checkpointer.save("model_final", iteration=self.iter)

    def train(self):
        self._t_after_step = time.perf_counter()     # `time` of the first iteration counts from here
        for self.iter in range(self.start_iter, self.max_iter):
            self.before_step()
            self.run_step()
            self.after_step()
        self.iter += 1


class ALDITrainer(DefaultTrainer):
    """Mean-Teacher trainer (aldi/trainer.py:140-246): builds student, EMA teacher and distiller; EMA tick before every step."""

    def _create_trainer(self, cfg, model, data_loader, optimizer):
        self.ema = EMA(build_aldi(cfg), cfg.EMA.ALPHA, cfg.EMA.START_ITER) if cfg.EMA.ENABLED else None
        distiller = build_distiller(cfg=cfg, teacher=self.ema.model if cfg.EMA.ENABLED else model, student=model)
        trainer = (ALDIAMPTrainer if cfg.SOLVER.AMP.ENABLED else ALDISimpleTrainer)(model, data_loader, optimizer, distiller,
                                                                                    backward_at_end=cfg.SOLVER.BACKWARD_AT_END,
                                                                                    model_batch_size=cfg.SOLVER.IMS_PER_GPU)
        trainer.fused = bool(cfg.SOLVER.get("FUSED_STEP", True)) and os.environ.get("ALDI_FUSED_STEP", "1") == "1"
        return trainer

    def _create_checkpointer(self, model, cfg):
        """aldi/trainer.py:151-156: EMA-aware start + the teacher as a checkpointable"""
        from .checkpoint import DetectionCheckpointer, DetectionCheckpointerWithEMA
        checkpointer = super()._create_checkpointer(model, cfg, ckpt_cls=DetectionCheckpointerWithEMA if cfg.EMA.LOAD_FROM_EMA_ON_START else DetectionCheckpointer)
        if cfg.EMA.ENABLED:
            checkpointer.add_checkpointable("ema", self.ema)
        return checkpointer

    @classmethod
    def build_model(cls, cfg):
        model = build_aldi(cfg)
        logging.getLogger(__name__).info("Model: %s", type(model).__mro__)
        return model

    @classmethod
    def build_optimizer(cls, cfg, model):
        if cfg.SOLVER.OPTIMIZER is None or cfg.SOLVER.OPTIMIZER.upper() == "SGD":
            if getattr(model, "adamw", False):
                raise ValueError("the ViTDet / ConvNeXt models are trained with SOLVER.OPTIMIZER ADAMW (their Base-RCNN-*.yaml)")
            return super(ALDITrainer, cls).build_optimizer(cfg, model)
        if cfg.SOLVER.OPTIMIZER.upper() == "ADAMW" and getattr(model, "detr", False):
            return EngineDetrAdamW(model, cfg)
        if cfg.SOLVER.OPTIMIZER.upper() == "ADAMW" and getattr(model, "adamw", False):       # reference aldi/trainer.py:200-209
            vitdet_b = cfg.MODEL.BACKBONE.NAME == "build_vitdet_b_backbone"          # include_vit_lr_decay of the reference
            return EngineAdamW(model, cfg.SOLVER.BASE_LR, lr_decay_rate=0.7 if vitdet_b else None, num_layers=12)
        raise ValueError(f"Unsupported optimizer/backbone combination {cfg.SOLVER.OPTIMIZER} {cfg.MODEL.BACKBONE.NAME}.")

    @classmethod
    def build_train_loader(cls, cfg):
        """Same batch-size arithmetic as the reference (aldi/trainer.py:211-240); the loaders are synthetic
        (datasets / decode / augmentation are outside the hot path: SURVEY.md section 8a row a20)."""
        contents, ratios = tuple(cfg.DATASETS.BATCH_CONTENTS), tuple(cfg.DATASETS.BATCH_RATIOS)
        if len(contents) != len(ratios):
            raise AssertionError("len(cfg.DATASETS.BATCH_CONTENTS) must equal len(cfg.DATASETS.BATCH_RATIOS).")
        total = cfg.SOLVER.IMS_PER_BATCH
        # every batch part gets its (truncated) share of the global batch; the shares must add up again
        # (a LIST, one entry per batch part: a content named twice counts twice, as in the reference's loop, aldi/trainer.py:211-222)
        sizes = [int(total * r / sum(ratios)) for r in ratios]
        if sum(sizes) != total:
            raise AssertionError(f"sum(batch_sizes)={sum(sizes)} must equal total_batch_size={total}")
        share = {}
        for part, n in zip(contents, sizes):
            share[part] = max(share.get(part, 0), n)
        # weak and strong views of one domain are cut from the same images: a domain's loader serves the larger of its parts
        labeled_bs = max((n for part, n in share.items() if part.startswith("labeled")), default=0)
        unlabeled_bs = max((n for part, n in share.items() if part.startswith("unlabeled")), default=0)
        batch_contents = contents
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        if cfg.DATASETS.get("FILES", False):
            return cls._build_file_train_loader(cfg, labeled_bs // world, unlabeled_bs // world, contents, rank, world)
        syn = cfg.get("SYNTHETIC", {})
        h, w = syn.get("HEIGHT", 800), syn.get("WIDTH", 1333)
        K = _num_classes(cfg)
        fixed = bool(syn.get("FIXED", False))
        labeled_loader = SyntheticDetectionLoader(labeled_bs // world, h, w, K, 1000 + 17 * rank, True, fixed=fixed) if labeled_bs > 0 else None
        unlabeled_loader = SyntheticDetectionLoader(unlabeled_bs // world, h, w, K, 2000 + 17 * rank, False, fixed=fixed) if unlabeled_bs > 0 else None
        device_strong, device_weak = bool(cfg.AUG.get("DEVICE_STRONG", False)), bool(cfg.AUG.get("DEVICE_WEAK", False))
        if device_strong or device_weak:
            # strong views from the reference's chain on the device (aldi/trainer.py:224-236 include_strong_augs: only for a
            # domain whose strong view the batch asks for), private draws seeded per rank and domain.  AUG.DEVICE_WEAK puts the
            # weak view's geometry (ResizeShortestEdge + RandomFlip of the loader's decoded image, aldi/aug.py:16-37) into the
            # same stage, ahead of the strong chain, with draws of its own
            from .aug import get_strong_augs, get_weak_augs
            base = max(int(cfg.SEED), 0)
            weak = get_weak_augs(cfg, True) if device_weak else None

            def stage(loader, labeled, part):
                return DeviceStrongAugLoader(loader, get_strong_augs(cfg, labeled) if device_strong and part in contents else None,
                                             device_strong_seed(base, rank, labeled), weak=weak,
                                             weak_seed=device_weak_seed(base, rank, labeled) if device_weak else None)
            if labeled_loader is not None:
                labeled_loader = stage(labeled_loader, True, "labeled_strong")
            if unlabeled_loader is not None:
                unlabeled_loader = stage(unlabeled_loader, False, "unlabeled_strong")
        return WeakStrongDataloader(labeled_loader, unlabeled_loader, batch_contents)

    # ---- DATASETS.FILES: the datasets on disk
    @staticmethod
    def _check_file_datasets(cfg, names):
        """DATASETS.FILES needs the device view (the host resizes nothing) and registered names (nothing is registered implicitly)"""
        from .datasets import DatasetCatalog
        if not cfg.AUG.get("DEVICE_WEAK", False):
            raise ValueError("DATASETS.FILES needs AUG.DEVICE_WEAK: the decoded images are cropped, resized and flipped on the device only")
        missing = [n for n in names if n not in DatasetCatalog]
        if missing:
            raise KeyError(f"DATASETS.FILES: not in the DatasetCatalog: {missing} (registered: {DatasetCatalog.list()}); register them "
                           "with aldi_amd.datasets.register_coco_instances / register_reference_datasets")

    @classmethod
    def _build_file_train_loader(cls, cfg, labeled_bs, unlabeled_bs, contents, rank, world):
        """the labeled loader reads DATASETS.TRAIN (DATALOADER.FILTER_EMPTY_ANNOTATIONS as in detectron2), the unlabeled one
        DATASETS.UNLABELED (nothing filtered, instances emptied); each is FileDetectionLoader -> the one device stage with the full
        chain `get_view_augs(cfg, True)`, so INPUT.CROP.* and INPUT.RANDOM_FLIP "vertical" work here"""
        from .aug import get_strong_augs, get_view_augs
        from .dataloader import FileDetectionLoader, TrainingSampler, file_sampler_seed
        from .datasets import get_detection_dataset_dicts
        from .mapper import DatasetMapper
        train, unl = list(cfg.DATASETS.TRAIN), list(cfg.DATASETS.UNLABELED)
        cls._check_file_datasets(cfg, (train if labeled_bs > 0 else []) + (unl if unlabeled_bs > 0 else []))
        for bs, names, key in ((labeled_bs, train, "TRAIN"), (unlabeled_bs, unl, "UNLABELED")):
            if bs > 0 and not names:
                raise ValueError(f"DATASETS.FILES: the batch asks for {key.lower()} images but DATASETS.{key} is empty")
        base = max(int(cfg.SEED), 0)
        device_strong = bool(cfg.AUG.get("DEVICE_STRONG", False))
        view = get_view_augs(cfg, True)
        threads = int(cfg.DATALOADER.NUM_WORKERS)

        def domain(bs, names, labeled, part):
            if bs <= 0:
                return None
            dicts = get_detection_dataset_dicts(names, filter_empty=bool(cfg.DATALOADER.FILTER_EMPTY_ANNOTATIONS) if labeled else False)
            if not dicts:
                raise ValueError(f"DATASETS.FILES: {names} have no images left after DATALOADER.FILTER_EMPTY_ANNOTATIONS")
            mapper = DatasetMapper(cfg, True, labeled)
            files = FileDetectionLoader(dicts, mapper, bs, TrainingSampler(len(dicts), True, file_sampler_seed(base, labeled), rank, world), threads)
            return DeviceStrongAugLoader(files, get_strong_augs(cfg, labeled) if device_strong and part in contents else None,
                                         device_strong_seed(base, rank, labeled), weak=view, weak_seed=device_weak_seed(base, rank, labeled),
                                         view=True, swap_rb=mapper.swap_rb)
        return WeakStrongDataloader(domain(labeled_bs, train, True, "labeled_strong"), domain(unlabeled_bs, unl, False, "unlabeled_strong"),
                                    contents)

    @classmethod
    def _build_file_test_loader(cls, cfg, dataset_name):
        """a lazy, finite loader over the registered dataset (one image per batch, this rank's InferenceSampler shard) + its records"""
        from .aug import get_view_augs
        from .dataloader import DeviceTestViewLoader, FileDetectionLoader, InferenceSampler
        from .datasets import DatasetCatalog
        from .mapper import DatasetMapper
        cls._check_file_datasets(cfg, [dataset_name])
        records = DatasetCatalog.get(dataset_name)
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        mapper = DatasetMapper(cfg, False, True)
        files = FileDetectionLoader(records, mapper, 1, InferenceSampler(len(records), rank, world), int(cfg.DATALOADER.NUM_WORKERS))
        return DeviceTestViewLoader(files, get_view_augs(cfg, False), mapper.swap_rb, cfg.MODEL.DEVICE), records

    def before_step(self):
        super(ALDITrainer, self).before_step()
        if self.cfg.EMA.ENABLED:
            t = self._trainer
            if getattr(t, "fused", False) and type(t.model.engine).__name__ == "RCNN":
                # the fused step runs the tick on the teacher's stream, beside the student's forward (only the teacher's
                # inference needs the new weights); `run_model` falls back to running it right away when it cannot fuse
                t._pending_ema = (self.ema, self.iter)
            else:
                self.ema.update_weights(t.model, self.iter)

    # ---- evaluation (reference aldi/trainer.py:166-196: COCO evaluator, EvalHook on the EMA model, BestCheckpointer on bbox/AP50)
    @classmethod
    def build_test_loader(cls, cfg, dataset_name):
        """synthetic validation split: a finite list of batches of {image, image_id, height, width} + detectron2-format records
        (DATASETS.FILES: a lazy loader over the registered dataset `dataset_name` and its records)"""
        if cfg.DATASETS.get("FILES", False):
            return cls._build_file_test_loader(cfg, dataset_name)
        syn_ = cfg.get("SYNTHETIC", {})
        h, w = syn_.get("HEIGHT", 800), syn_.get("WIDTH", 1333)
        n, K = int(syn_.get("VAL_IMAGES", 8)), _num_classes(cfg)
        g = torch.Generator().manual_seed(4242)
        batches, records = [], []
        weak = None
        if cfg.AUG.get("DEVICE_WEAK", False):
            # detectron2's test-time mapper: ResizeShortestEdge at MIN_SIZE_TEST / MAX_SIZE_TEST, no flip and nothing drawn; the
            # records keep the raw height / width, so the evaluators' rescaling brings the detections back
            from . import aug
            weak = aug.get_weak_augs(cfg, False)[0]
            size = weak.short_edge_length[0]
        for i in range(n):
            img, inst = synthetic.make_image(h, w, int(torch.randint(5, 21, (1,), generator=g)), K, g)
            if weak is not None and size != 0:
                nh, nw = weak.get_output_shape(h, w, size, weak.max_size)
                img = aug.weak_views([img.to(cfg.MODEL.DEVICE).contiguous()], [aug.WeakParams(h, w, nh, nw, False)], chw_out=True, chw_in=True)[0]
            batches.append([{"image": img, "image_id": i, "height": h, "width": w}])
            records.append(dict(image_id=i, height=h, width=w,
                                annotations=[dict(bbox=b.tolist(), bbox_mode="XYXY_ABS", category_id=int(c))
                                             for b, c in zip(inst["gt_boxes"], inst["gt_classes"])]))
        return batches, records

    @classmethod
    def build_evaluator(cls, cfg, dataset_name, output_folder=None, dataset_dicts=None):
        """Just do COCO Evaluation (`TEST.DEVICE_EVAL`: matched and accumulated on the device, same numbers)."""
        from .evaluation import Detectron2COCOEvaluatorAdapter, DeviceCOCOEvaluator
        if output_folder is None:
            output_folder = os.path.join(cfg.OUTPUT_DIR, "inference")
        detail = bool(cfg.TEST.get("EVAL_DETAIL", False))        # AR, per-class AP, precision / recall above the teacher's score cut
        kw = dict(output_dir=output_folder, detail=detail, score_thresh=cfg.DOMAIN_ADAPT.TEACHER.THRESHOLD if detail else None)
        ev = DeviceCOCOEvaluator if cfg.TEST.get("DEVICE_EVAL", False) else Detectron2COCOEvaluatorAdapter
        return ev(dataset_name, dataset_dicts or [], _num_classes(cfg), **kw)

    @classmethod
    def test(cls, cfg, model, evaluators=None):
        """detectron2 DefaultTrainer.test: {dataset: {"bbox": {...}}} (flattened to the single dict when there is one dataset)"""
        from .evaluation import inference_on_dataset
        names = list(cfg.DATASETS.TEST) or ["synthetic_val"]
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        results = OrderedDict()
        for i, name in enumerate(names):
            loader, records = cls.build_test_loader(cfg, name)
            ev = evaluators[i] if evaluators is not None else cls.build_evaluator(cfg, name, dataset_dicts=records)
            # detectron2's InferenceSampler: every rank runs a disjoint shard of the test set, the evaluator gathers the
            # predictions on rank 0 (each detection counted once; the ground truth stays the full set)
            results[name] = inference_on_dataset(model, loader[rank::world] if world > 1 and isinstance(loader, list) else loader, ev)   # (a file loader shards itself)
        return results[names[0]] if len(results) == 1 else results

    @classmethod
    def test_with_TTA(cls, cfg, model):
        """detectron2 tools/train_net.py `Trainer.test_with_TTA`: the model wrapped in GeneralizedRCNNWithTTA (aldi_amd/tta.py), evaluators
        writing to <OUTPUT_DIR>/inference_TTA, result keys suffixed "_TTA".  The wrapper's Instances are in the original image's
        coordinates with image_size = (height, width), so the evaluators' rescaling is by exactly 1."""
        from .tta import GeneralizedRCNNWithTTA
        logging.getLogger(__name__).info("Running inference with test-time augmentation ...")
        wrapped = GeneralizedRCNNWithTTA(cfg, model)
        names = list(cfg.DATASETS.TEST) or ["synthetic_val"]
        folder = os.path.join(cfg.OUTPUT_DIR, "inference_TTA")
        evaluators = [cls.build_evaluator(cfg, name, output_folder=folder, dataset_dicts=cls.build_test_loader(cfg, name)[1]) for name in names]
        res = cls.test(cfg, wrapped, evaluators)
        return OrderedDict({k + "_TTA": v for k, v in res.items()})

    def after_step(self):
        """aldi/trainer.py:173-196: EvalHook on the EMA model (the student without EMA) every TEST.EVAL_PERIOD iterations and
        after the last one; BestCheckpointer on `bbox/AP50` (one test set) or `<test_set>/bbox/AP50` (several), "max",
        written as `<test_set>_model_best.pth` by the main process."""
        super(ALDITrainer, self).after_step()
        period = self.cfg.TEST.EVAL_PERIOD
        last = self.iter >= self.max_iter - 1
        if period > 0 and ((self.iter + 1) % period == 0 or last):
            self.flush_metrics()                     # before the evaluation and `_model_best`: a non-finite loss raises here
            self._last_eval_results = self.test(self.cfg, self.ema.model if self.cfg.EMA.ENABLED else self.model)
            names = list(self.cfg.DATASETS.TEST) or ["synthetic_val"]
            if not self._is_main_process():
                return
            best = self.__dict__.setdefault("_best_ap50", {})
            for name in names:
                res = self._last_eval_results if len(names) == 1 else self._last_eval_results.get(name, {})
                ap50 = res.get("bbox", {}).get("AP50", float("nan"))
                if ap50 == ap50 and ap50 > best.get(name, float("-inf")):
                    best[name] = ap50
                    self.checkpointer.save(f"{name}_model_best", iteration=self.iter)


Trainer = ALDITrainer   # BASELINE.json calls it aldi.trainer.Trainer

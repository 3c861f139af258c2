"""Plain Point-MAE pre-training: the model the published GM3D run distils from (its frozen teacher) and the baseline the paper
compares against.  Host-side mirror of the reference's Point-MAE_SA3D/tools/runner_pretrain.py::run_net (P/tools/ below, :58-208)
with tools/builder.py::build_opti_sche (:38-90) and ::save_checkpoint (:128-137).

  augment (PointcloudScaleAndTranslate) -> Point_MAE.forward (mask, encoder on the visible groups, decoder, Chamfer loss on the
  masked patches) -> backward -> every `step_per_update` iterations: AdamW step, zero_grad.

run_net has NO gradient clipping and NO EMA teacher, so neither exists here: the flat optimizer runs with max_norm = 0 (its
kernel then leaves the gradients unscaled) and without a teacher.  Nothing in an iteration talks to the host: the mask comes from
gm3d_mask_centers (MaskTransformer.device_mask), the loss from the fused patch kernels, the learning rate is a device scalar, and
the whole iteration replays as one hipGraph (engine_pretrain.GraphedPretrainStep through its fwd_bwd= / extra= hooks).
Out of scope: data-parallel training, SyncBatchNorm, `vis=True` plotting, datasets.
"""
import math
import time
import weakref
from contextlib import nullcontext
from types import SimpleNamespace

import torch

from . import engine_pretrain as E
from . import streams
from .engine_pretrain import train_transforms  # noqa: F401 (part of this module's interface, like the sibling engines)


# --------------------------------------------------------------------------- optimizer / schedule
def build_optimizer(model, lr=1e-3, weight_decay=0.05, flat=True, capturable=False):
    """AdamW of cfgs/config.yaml (lr 1e-3, weight decay 0.05) with the reference's grouping (P/tools/builder.py:40-56: no decay
    when param.ndim == 1, the name ends in `.bias` or contains `token`).  flat=True: FlatAdamWEma without a teacher and without
    clipping (GPU only; what the captured step needs); otherwise torch.optim.AdamW over [no_decay, decay]."""
    if flat:
        from .optim import FlatAdamWEma
        return FlatAdamWEma(model, None, lr=lr, weight_decay=weight_decay, max_norm=0.0)
    return E.build_optimizer(model, lr=lr, weight_decay=weight_decay, flat=False, capturable=capturable)


def cosine_lr(epoch, base_lr=1e-3, epochs=300, warmup_epochs=10, lr_min=1e-6, warmup_lr_init=1e-6):
    """CosineLRScheduler(t_initial=epochs, t_mul=1, lr_min=1e-6, decay_rate=0.1, warmup_lr_init=1e-6, warmup_t=warmup_epochs,
    cycle_limit=1, t_in_epochs=True) of build_opti_sche, evaluated at t = epoch:
        t <  warmup_epochs:  warmup_lr_init + t * (base_lr - warmup_lr_init) / warmup_epochs
        t <  epochs:         lr_min + (base_lr - lr_min) / 2 * (1 + cos(pi * t / epochs))     (no warm-up prefix: t is NOT shifted, so
                             the peak, reached at t = warmup_epochs, is the cosine's value there -- base_lr up to the factor
                             (1 + cos(pi * warmup_epochs / epochs)) / 2, 0.9973 for 10 / 300)
        t >= epochs:         lr_min                                                           (cycle_limit = 1)
    timm is not available where this was written: the closed form is restated from timm 0.4.5's scheduler/cosine_lr.py and is NOT
    pinned by a fixture."""
    t = epoch
    if t < warmup_epochs:
        return warmup_lr_init + t * (base_lr - warmup_lr_init) / warmup_epochs
    if t >= epochs:
        return lr_min
    return lr_min + 0.5 * (base_lr - lr_min) * (1.0 + math.cos(math.pi * t / epochs))


def set_lr(optimizer, lr):
    """lr -> every parameter group; a device scalar (flat / capturable optimizers) is filled in place, so a captured step sees it."""
    for group in optimizer.param_groups:
        if isinstance(group["lr"], torch.Tensor):
            group["lr"].fill_(lr)
        else:
            group["lr"] = lr
    return lr


def lr_for_epoch(epoch, args):
    """run_net calls scheduler.step(epoch) AFTER epoch `epoch` (P/tools/:176-180): epoch e > 0 trains at the schedule's value for
    t = e - 1, epoch 0 at warmup_lr_init (what the scheduler's constructor writes)."""
    return cosine_lr(max(epoch - 1, 0), getattr(args, "lr", 1e-3), getattr(args, "epochs", 300), getattr(args, "warmup_epochs", 10))


# --------------------------------------------------------------------------- the step
def _accum(args):
    return int(getattr(args, "step_per_update", getattr(args, "accum_iter", 1)))


def step_forward_backward(model, model_ema, samples, epoch, args, grad_sync=None, mask_noise=None, mask_start=None, augment=True,
                          aug_draws=None, optimizer=None, accum_first=True, accum_last=True, generator=None):
    """augment -> loss -> backward (P/tools/:137-144), in the calling convention of engine_pretrain.GraphedPretrainStep's fwd_bwd=
    hook (model_ema, epoch and grad_sync are part of that convention and unused: there is no teacher, no epoch-dependent mask and
    no data-parallel form).  Gradients are SUMMED over a step_per_update window, like the reference's repeated backward()."""
    raw = model.module if hasattr(model, "module") else model
    if augment:
        samples = train_transforms(samples, draws=aug_draws, generator=generator)
    bf16 = getattr(args, "bf16", False)
    if bf16:
        from .fused import weight_cache
        weight_cache.pin(raw)        # no-op after the first call
        weight_cache.refresh()
    enc = raw.MAE_encoder
    if mask_noise is None and mask_start is None and not enc.device_mask:
        raise RuntimeError("the Point-MAE engine masks on the device: set model.MAE_encoder.device_mask = True (or inject the draws)")
    rand = enc.mask_type == "rand"
    with (torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else nullcontext()):
        loss = model(samples, mask_noise=mask_noise if rand else None, mask_start=None if rand else mask_start)
    E.backward_and_collect(loss, raw, optimizer, None, _accum(args), accum_first, accum_last, async_w=False)
    return {"loss": loss.detach()}


def pretrain_step(model, optimizer, samples, args=None, mask_noise=None, mask_start=None, augment=True, aug_draws=None,
                  micro_step=None, generator=None):
    """One iteration of run_net's loop (P/tools/:137-151), eager.  `samples` (B,N,3) f32 on the GPU (augmented in place).  Returns
    device tensors only.  step_per_update > 1 needs micro_step (the iteration index inside the epoch): the optimizer steps, and
    the gradients are cleared, when (micro_step + 1) % step_per_update == 0; other iterations return grad_norm = None."""
    args = args if args is not None else SimpleNamespace()
    accum = _accum(args)
    if accum > 1 and micro_step is None:
        raise ValueError("step_per_update = %d needs micro_step (the iteration index) to place the update" % accum)
    first = accum == 1 or micro_step % accum == 0
    last = accum == 1 or (micro_step + 1) % accum == 0
    out = step_forward_backward(model, None, samples, 0, args, mask_noise=mask_noise, mask_start=mask_start, augment=augment,
                                aug_draws=aug_draws, optimizer=optimizer, accum_first=first, accum_last=last, generator=generator)
    out["grad_norm"] = None
    if last:
        if hasattr(optimizer, "flat_grad_views"):
            out["grad_norm"] = E.step_update(model, None, optimizer)
        else:
            optimizer.step()          # no clipping in run_net
    return out


class GraphedPointMAEStep(E.GraphedPretrainStep):
    """The iteration as one hipGraph (two with step_per_update > 1: forward + backward + GA += G | AdamW, the captured-accumulation
    layout of GraphedPretrainStep).  Needs the flat optimizer.  inject_mask_noise=True: the ranking noise (rand) or the start
    indices (block) are static inputs filled by the caller -- deterministic replays for the tests; otherwise they are drawn inside
    the graph."""

    def __init__(self, model, optimizer, example, args=None, warmup_iters=3, augment=True, inject_mask_noise=False, generator=None):
        if not hasattr(optimizer, "flat_grad_views"):
            raise NotImplementedError("the captured Point-MAE step needs the flat optimizer (build_optimizer(flat=True))")
        raw = model.module if hasattr(model, "module") else model
        a = SimpleNamespace(bf16=getattr(args, "bf16", False), accum_iter=_accum(args) if args is not None else 1)
        self.block = raw.MAE_encoder.mask_type != "rand"
        self.static_start = None
        if inject_mask_noise and self.block:
            self.static_start = torch.zeros(example.shape[0], dtype=torch.int32, device=example.device)
        extra = {"mask_start": self.static_start, "generator": generator}
        super().__init__(model, None, optimizer, a, example, 0, warmup_iters=warmup_iters, augment=augment,
                         inject_mask_noise=inject_mask_noise and not self.block, fwd_bwd=step_forward_backward, extra=extra)

    def __call__(self, samples, mask_noise=None, mask_start=None, update=True):
        if self.static_start is not None:
            self.static_start.copy_(mask_start, non_blocking=True)
        return super().__call__(samples, mask_noise=mask_noise, update=update)


# --------------------------------------------------------------------------- the epoch loop
_warm = weakref.WeakKeyDictionary()      # model -> eager iterations run so far in this process
_steps = weakref.WeakKeyDictionary()     # model -> its captured step (the graph reads lr from the device: it outlives the epoch)


def train_one_epoch(model, data_loader, optimizer, device, epoch, args, log_writer=None, print_freq=20, use_graph=None):
    """One epoch of run_net's loop (P/tools/:106-187).  The loader yields (B,N,3) float batches.  -> the averaged stats: `loss`
    (x 1000, like run_net's AverageMeter), `lr`, and the execution record (step_losses: every iteration's loss as computed,
    replayed_iters, capture_s, clouds_per_s).

    Execution: masking on the device (device_mask is switched on); the process's first engine_pretrain.EAGER_WARMUP_ITERS windows
    run eagerly, then the step is captured once and replayed, the next batch being copied to the device while the current one
    trains; a batch of another shape (a smaller last batch) runs eagerly.  The finite-loss guard is a device flag read every
    print_freq iterations and at the end.  use_graph=False (or a torch optimizer) keeps every iteration eager."""
    device = torch.device(device)
    raw = model.module if hasattr(model, "module") else model
    raw.MAE_encoder.device_mask = True
    model.train(True)
    accum = _accum(args)
    flat = hasattr(optimizer, "flat_grad_views")
    if use_graph is None:
        use_graph = flat and device.type == "cuda"
    lr = set_lr(optimizer, lr_for_epoch(epoch, args))
    if getattr(optimizer, "GA", None) is not None:      # a window the previous epoch left unfinished is discarded (num_iter = 0, P/tools/:117)
        optimizer.GA.zero_()
    optimizer.zero_grad()
    loader = streams.LookAhead(data_loader, lambda batch: batch.to(device, non_blocking=True))
    n_iter = len(loader)
    losses = torch.zeros(max(n_iter, 1), dtype=torch.float32, device=device)
    graphed = _steps.get(model) if use_graph else None
    n_replay, t_capture, seen = 0, 0.0, 0
    t0 = time.time()
    for it, samples in enumerate(loader):
        if (use_graph and graphed is None and it % accum == 0 and _warm.get(model, 0) >= E.EAGER_WARMUP_ITERS * accum):
            tc = time.time()
            graphed = _steps[model] = GraphedPointMAEStep(model, optimizer, samples, args, warmup_iters=0)
            t_capture = time.time() - tc
        last = (it + 1) % accum == 0
        if graphed is not None and samples.shape == graphed.static_in.shape:
            out = graphed(samples, update=last)
            n_replay += 1
        else:
            out = pretrain_step(model, optimizer, samples, args, micro_step=it)
            _warm[model] = _warm.get(model, 0) + 1
        losses[it] = out["loss"]
        seen += samples.shape[0]
        if (it + 1) % print_freq == 0:
            cur = losses[:it + 1]
            if not bool(torch.isfinite(cur).all()):     # one sync per print_freq
                raise FloatingPointError("non-finite loss in epoch %d near iteration %d" % (epoch, it))
            print("[Epoch %d][Batch %d/%d] Losses = %.4f lr = %.6f" % (epoch, it + 1, n_iter, float(cur.mean()) * 1000.0, lr))
    host = losses[:n_iter].tolist()          # the epoch's one synchronisation
    t1 = time.time()
    if any(not math.isfinite(v) for v in host):
        raise FloatingPointError("non-finite loss in epoch %d" % epoch)
    stats = {"loss": 1000.0 * sum(host) / max(len(host), 1), "lr": lr, "step_losses": host, "replayed_iters": n_replay,
             "capture_s": t_capture, "clouds_per_s": seen / max(t1 - t0, 1e-9)}
    if log_writer is not None:
        log_writer.add_scalar("Loss/Epoch/Loss_1", stats["loss"], epoch)
        log_writer.add_scalar("Loss/Epoch/LR", lr, epoch)
    return stats


# --------------------------------------------------------------------------- checkpoints
def save_checkpoint(path, model, optimizer, epoch, metrics=None, best_metrics=None):
    """builder.save_checkpoint's layout (P/tools/builder.py:128-137): {base_model, optimizer, epoch, metrics, best_metrics}, tensors
    and plain containers only (checkpoint.read_checkpoint / torch.load(weights_only=True) read it).  The file loads with
    PointTransformer.load_model_from_ckpt(key="base_model") and as the published run's frozen teacher (load_teacher)."""
    import os
    from .checkpoint import _cpu, _plain
    raw = model.module if hasattr(model, "module") else model
    d = {"base_model": _cpu(raw.state_dict()), "optimizer": _plain(optimizer.state_dict()) if optimizer is not None else {},
         "epoch": int(epoch), "metrics": dict(metrics or {}), "best_metrics": dict(best_metrics or {})}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = path + ".tmp"
    torch.save(d, tmp)
    os.replace(tmp, path)
    return path


def load_teacher(path, model):
    """`base_model` of a checkpoint -> a Point_MAE, frozen and in eval mode: the teacher of engine_pretrain_Classifier_SVM
    (P/main_pretrain.py:302-328).  Strict: every key must be there."""
    from .checkpoint import read_checkpoint
    sd = read_checkpoint(path)["base_model"]
    model.load_state_dict({k.replace("module.", ""): v for k, v in sd.items()}, strict=True)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.eval()

"""Point-M2AE + GeoMask3D pretraining epoch: the reference's train_one_epoch (Point-MAE_SA3D/engine_pretrain.py:38-271, which
main_pretrain.py runs for config_Point_M2AE.yaml) around the hierarchical model of point_m2ae.py.

The loop itself is engine_pretrain.run_epoch -- per-iteration learning rate, EMA-decay ramp, finite-loss guard, logging, the
eager warm-up iterations, one capture per epoch and the eager fallback for a batch of another shape are shared with Point-MAE.
This module supplies the Point-M2AE iteration:
  * one GPU: point_m2ae.GraphedM2AEStep (training graph + the next batch's grouping graph on a second stream, look-ahead fed from
    the loader);
  * a process group of N > 1 ranks: point_m2ae.SegmentedM2AEStep (four backward segments, each segment's all-reduce behind the
    next segment's backward), the optimizer laid out by point_m2ae.ddp_segment;
  * the augmentation draws from a generator of its own, seeded args.seed + rank (the reference seeds every rank that way,
    main_pretrain.py:200-202), so that they never share Philox offsets with the training graph's draws;
  * the visible-first overflow flag (a too-small static bound drops tokens) is read where the finite-loss guard is read.
"""
import weakref

import torch
import torch.distributed as dist

from . import engine_pretrain as E
from . import point_m2ae as P
from . import streams

_generators = weakref.WeakKeyDictionary()   # model -> its augmentation generator (kept across epochs: fresh draws every epoch)


def build_optimizer(model, lr=1e-3, weight_decay=0.05, ema_decay=0.999, clip_grad=5.0, segmented=None):
    """-> (FlatAdamWEma, ModelEma): the optimizer of config_Point_M2AE.yaml (AdamW, lr 1e-3, weight decay 0.05, the reference's
    no-decay rule) with clip(5) and the EMA teacher in the same pass.  segmented (default: a process group of > 1 ranks is alive):
    lay the flat buffers out by point_m2ae.ddp_segment, as the data-parallel step needs."""
    if segmented is None:
        segmented = dist.is_initialized() and dist.get_world_size() > 1
    model_ema = E.ModelEma(model, ema_decay)          # before the optimizer: it re-points the teacher's parameters into its buffer
    opt = E.build_optimizer(model, lr=lr, weight_decay=weight_decay, flat=True, model_ema=model_ema, clip_grad=clip_grad,
                            segment_of=P.ddp_segment if segmented else None)
    return opt, model_ema


def check_setup(optimizer, args, world):
    """The configurations this engine runs; raises otherwise."""
    accum = getattr(args, "accum_iter", 1)
    if accum > 1:
        raise NotImplementedError("Point-M2AE pretraining runs accum_iter = 1 (config_Point_M2AE.yaml: step_per_update 1), got %d" % accum)
    if world > 1:
        ranges = getattr(optimizer, "segment_ranges", None)
        if ranges is None or sorted(ranges) != list(range(P.SegmentedM2AEStep.NSEG)):
            raise ValueError("a process group of %d ranks trains with SegmentedM2AEStep: build the optimizer with "
                             "engine_pretrain_m2ae.build_optimizer(..., segmented=True) (FlatAdamWEma, segment_of=point_m2ae.ddp_segment)"
                             % world)


def augment_generator(model, device, args):
    """the model's augmentation generator, created on first use with seed args.seed + rank."""
    g = _generators.get(model)
    if g is None:
        rank = dist.get_rank() if dist.is_initialized() else 0
        g = torch.Generator(device=device)
        g.manual_seed(int(getattr(args, "seed", 0)) + rank)
        _generators[model] = g
    return g


def _as_run_epoch_out(out, device):
    """Point-M2AE's outputs as the vector run_epoch logs: loss + loss_learn = the objective (Chamfer + ranking loss); this model has
    no MSE term.  vis_overflow travels along for the guard."""
    res = {"loss": out["loss_chfr"], "loss_learn": out["loss_learn"], "loss_chfr": out["loss_chfr"],
           "loss_mse": E._const_scalar(device, 0.0), "grad_norm": out["grad_norm"]}
    if out.get("vis_overflow") is not None:
        res["vis_overflow"] = out["vis_overflow"]
    return res


class _Replayed:
    """run_epoch's view of a captured step: step(samples, update=) with `static_in`; the look-ahead comes from the loader."""

    def __init__(self, step, lookahead, device):
        self.step, self.lookahead, self.device = step, lookahead, device
        self.static_in = step.static_in

    def __call__(self, samples, update=True):
        nxt = self.lookahead.next
        if nxt is not None and nxt.shape != self.static_in.shape:
            nxt = None                     # the next batch runs eagerly (run_epoch's fallback): nothing to stage for it
        return _as_run_epoch_out(self.step(samples, next_pts=nxt), self.device)


def train_one_epoch(model, data_loader, optimizer, device, epoch, loss_scaler=None, log_writer=None, args=None, model_ema=None,
                    model_teacher=None, scheduler=None, optimizer_learn_loss=None, print_freq=20, use_graph=None, generator=None):
    """Drop-in for P/engine_pretrain.py::train_one_epoch with the Point-M2AE model (same positional arguments; `loss_scaler`,
    `model_teacher`, `scheduler`, `optimizer_learn_loss` are accepted for signature compatibility).  The loader yields this rank's
    (B,N,3) float batches.  -> the epoch's averaged stats (loss, loss_learn, loss_mse = 0, loss_chfr, grad_norm, lr) plus
    run_epoch's execution record (replayed_iters, capture_s, clouds/s).

    Execution: the first engine_pretrain.EAGER_WARMUP_ITERS iterations of the process run eagerly, then every epoch captures its
    step once and replays it: GraphedM2AEStep on one GPU, SegmentedM2AEStep with a process group of > 1 ranks (optimizer from
    build_optimizer(..., segmented=True)).  use_graph=False (or a torch optimizer) keeps every iteration eager.
    generator: the augmentation generator (default: one per model, seeded args.seed + rank)."""
    assert model_ema is not None, "Point-M2AE + GeoMask3D trains with the EMA teacher"
    device = torch.device(device)
    world = dist.get_world_size() if dist.is_initialized() else 1
    check_setup(optimizer, args, world)
    flat = hasattr(optimizer, "flat_grad_views")
    if world > 1 and not flat:
        raise ValueError("data-parallel Point-M2AE needs the flat optimizer (engine_pretrain_m2ae.build_optimizer)")
    model.train(True)
    model_ema.decay = E.ema_decay_for_epoch(epoch)
    if use_graph is None:
        use_graph = flat and device.type == "cuda"
    gen = generator if generator is not None else augment_generator(model, device, args)
    divider = model_ema.ema.group_divider
    if device.type == "cuda":
        from . import masked_stack
        masked_stack.overflow_flag(device).zero_()       # this epoch's overflow only (the kernels never clear it)
    loader = streams.LookAhead(data_loader, lambda batch: batch.to(device, non_blocking=True))
    if world > 1 and not getattr(optimizer, "_m2ae_broadcast", False):
        # DDP's constructor: rank 0's parameters, optimizer state, teacher and buffers (the ranks were seeded differently)
        E.broadcast_state(model, model_ema, optimizer)
        optimizer._m2ae_broadcast = True

    def eager_step(samples, it):
        if world > 1:
            seg = getattr(optimizer, "_m2ae_eager_step", None)
            if seg is None:
                seg = optimizer._m2ae_eager_step = P.SegmentedM2AEStep(model, model_ema, optimizer, args, samples, epoch,
                                                                       generator=gen, use_graphs=False, broadcast=False)
            seg.epoch, seg.generator = epoch, gen
            out = seg(samples.clone())
        else:
            staged = P.group_stage(divider, samples.clone(), augment=True, generator=gen)
            out = P.pretrain_step(model, model_ema, optimizer, None, epoch, args, staged=staged)
        return _as_run_epoch_out(out, device)

    def capture(example):
        if world > 1:
            step = P.SegmentedM2AEStep(model, model_ema, optimizer, args, example, epoch, warmup_iters=0, generator=gen,
                                       broadcast=False)
        else:
            step = P.GraphedM2AEStep(model, model_ema, optimizer, args, example, epoch, warmup_iters=0, generator=gen)
        return _Replayed(step, loader, device)

    return E.run_epoch(loader, optimizer, device, epoch, args, eager_step, capture, log_writer=log_writer, print_freq=print_freq,
                       model_key=model, use_graph=use_graph)

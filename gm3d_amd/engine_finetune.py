"""Fine-tune / classification step: Point-MAE_SA3D/engine_finetune.py:70-176 (train_one_epoch),
:179-215 (evaluate) and the optimizer set-up of main_finetune.py:357-365 (layer-wise lr decay, util/lr_decay.py).

Per iteration, all on the GPU: FPS 8192 -> point_all (1200 for npoints 1024) with the HIP FPS kernel, ONE host-drawn
random subset of `npoints` of those indices shared by the batch (np.random.choice, like the reference), gather,
scale-and-translate augmentation, PointTransformer forward under bf16 autocast, cross-entropy, backward,
gradient clipping, AdamW.  The reference runs fp16 autocast + GradScaler; bf16 needs no loss scaling, so the
`loss_scaler` argument is accepted for signature compatibility and only its clip/step duty is performed.

Soft targets (gm3d_amd/losses.py) are opt-in: build_criterion picks the smoothed loss a model's config or the driver's --smoothing asks
for, and `mixup=PointMixup(alpha)` mixes the batch after train_transforms, where the reference's (commented) call stands
(P/engine_finetune.py:136-137).  Host draws of one iteration, in this order: the FPS subset (np.random.choice), then the mixup's
lam (rng.beta) and permutation (torch.randperm) -- the reference's.  With neither, every path issues the launches it always did.
"""
import math
import sys

import numpy as np
import torch

from . import ops
from . import streams
from .engine_pretrain import train_transforms

POINT_ALL = {1024: 1200, 2048: 2400, 4096: 4800, 8192: 8192}


# --------------------------------------------------------------------------- optimizer (util/lr_decay.py)
def get_layer_id_for_vit(name, num_layers):
    """P/util/lr_decay.py:65-78.  For this model: cls_token -> 0, blocks.blocks.{i}.* -> i + 1, everything else
    (encoder.*, pos_embed.*, cls_pos, norm_p.*, cls_head_finetune.*) -> num_layers."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[2]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=0.75, num_layers=12):
    """Layer-wise lr decay groups (P/util/lr_decay.py:15-62): lr_scale = layer_decay ** (num_layers - layer_id);
    1-D parameters (and exact names in `no_weight_decay_list`) get weight_decay 0."""
    scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    groups = {}
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        no_decay = p.ndim == 1 or n in no_weight_decay_list
        lid = get_layer_id_for_vit(n, num_layers)
        key = "layer_%d_%s" % (lid, "no_decay" if no_decay else "decay")
        if key not in groups:
            groups[key] = {"lr_scale": scales[lid], "weight_decay": 0.0 if no_decay else weight_decay, "params": [],
                           "names": []}
        groups[key]["params"].append(p)
        groups[key]["names"].append(n)
    return list(groups.values())


def build_optimizer(model, lr, weight_decay=0.05, layer_decay=0.75, capturable=False, flat=False, max_norm=None,
                    num_layers=12):
    """torch.optim.AdamW(param_groups_lrd(...), lr) as in P/main_finetune.py:359-365 (multi-tensor fused update).
    capturable=True: per-group learning rates live in device tensors (hipGraph capture).
    flat=True: the same update (same groups: lr_scale per layer, no weight decay for 1-D parameters) as ONE pass over flat
    buffers -- optim.FlatAdamWEma with a per-element lr multiplier; gradient clipping (`max_norm`) happens inside its
    step, the learning rate is a device scalar (graph-capturable), and the GEMMs read the bf16 shadows it maintains."""
    if flat:
        from .optim import FlatAdamWEma
        scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
        return FlatAdamWEma(model, None, lr=lr, weight_decay=weight_decay, max_norm=max_norm if max_norm else 0.0,
                            no_decay_of=lambda n, p: p.ndim == 1,
                            lr_scale_of=lambda n: scales[get_layer_id_for_vit(n, num_layers)])
    groups = [{k: v for k, v in g.items() if k != "names"} for g in param_groups_lrd(
        model, weight_decay, no_weight_decay_list=[{"pos_embed", "cls_token"}], layer_decay=layer_decay)]
    dev = next(model.parameters()).device
    kw = {"fused": True} if dev.type == "cuda" else {}
    if capturable:
        kw["capturable"] = True
        for g in groups:
            g["lr"] = torch.tensor(float(lr), dtype=torch.float32, device=dev)
    return torch.optim.AdamW(groups, lr=lr, **kw)


def adjust_learning_rate(optimizer, epoch, args):
    """P/util/lr_sched.py:11-23 with the per-group lr_scale."""
    if epoch < args.warmup_epochs:
        lr = args.lr * epoch / args.warmup_epochs
    else:
        lr = args.min_lr + (args.lr - args.min_lr) * 0.5 * \
            (1.0 + math.cos(math.pi * (epoch - args.warmup_epochs) / (args.epochs - args.warmup_epochs)))
    for g in optimizer.param_groups:
        v = lr * g["lr_scale"] if "lr_scale" in g else lr
        if torch.is_tensor(g["lr"]):
            g["lr"].fill_(v)                      # capturable optimizer: the captured update reads this tensor
        else:
            g["lr"] = v
    return lr


# --------------------------------------------------------------------------- the criterion
def _model_smooth(model):
    """The `smooth` of the model's config (Point-M2AE's fine-tune yamls), or 0."""
    config = getattr(getattr(model, "module", model), "config", None)
    if config is None:
        return 0.0
    v = config.get("smooth", 0.0) if isinstance(config, dict) else getattr(config, "smooth", 0.0)
    return float(v or 0.0)


def build_criterion(model=None, args=None):
    """The switch of P/main_finetune.py:369-375 (commented out upstream), as an opt-in helper: SmoothLoss(smooth) when the model's
    config sets `smooth` (Point-M2AE_SA3D/cfgs/finetune_modelnet_PointM2AE.yaml:73), else LabelSmoothingCrossEntropy(args.smoothing) when
    that is positive, else nn.CrossEntropyLoss().  Mixup needs no criterion of its own: both smoothed losses take MixedTargets."""
    from .losses import LabelSmoothingCrossEntropy, SmoothLoss
    smooth = _model_smooth(model)
    if smooth > 0.0:
        return SmoothLoss(smooth)
    smoothing = float(getattr(args, "smoothing", 0.0) or 0.0)
    if smoothing > 0.0:
        return LabelSmoothingCrossEntropy(smoothing)
    return torch.nn.CrossEntropyLoss()


def _check_mixup(mixup):
    """None or a losses.PointMixup.  timm's image Mixup cannot mix point clouds (and upstream's call site for it names an undefined
    variable), so anything else is refused rather than ignored."""
    if mixup is None:
        return None
    from .losses import PointMixup
    if not isinstance(mixup, PointMixup):
        raise TypeError("mixup must be None or a gm3d_amd.losses.PointMixup, not %s" % type(mixup).__name__)
    return mixup


# --------------------------------------------------------------------------- the step
def sample_points(points, npoints, subset=None, rng=np.random):
    """P/engine_finetune.py:117-134: FPS to point_all, keep a random `npoints`-subset of the FPS order (the same
    subset for every cloud of the batch), gather.  `subset` injects the index draw (parity tests)."""
    if npoints not in POINT_ALL:
        raise NotImplementedError("npoints %d" % npoints)
    point_all = min(POINT_ALL[npoints], points.size(1))
    fps_idx = ops.furthest_point_sample(points.contiguous(), point_all)                 # (B, point_all) int32
    if subset is None:
        subset = rng.choice(point_all, npoints, False)
    if not torch.is_tensor(subset):                     # a device LongTensor is used as is (graph capture: static input)
        subset = torch.as_tensor(np.asarray(subset), dtype=torch.long).to(points.device)
    fps_idx = fps_idx.index_select(1, subset).contiguous()
    return ops.gather_operation(points.transpose(1, 2).contiguous(), fps_idx).transpose(1, 2).contiguous()


def finetune_step(model, criterion, optimizer, points, targets, npoints=1024, max_norm=None, bf16=True, subset=None,
                  aug_draws=None, augment=True, update=True, accum_iter=1, presampled=False, mixup=None, mixup_drawn=False):
    """One iteration of P/engine_finetune.py:108-151.  points (B,N0,3) f32 and targets (B,) on the GPU.
    presampled=True: `points` already is the (B,npoints,3) output of sample_points (sampling overlapped elsewhere).
    mixup: a losses.PointMixup applied after train_transforms -- its host draw (lam, permutation) is made here, after the subset's,
    unless mixup_drawn (the caller staged it with mixup.draw: the captured step, parity tests); the criterion then receives
    MixedTargets.  None: today's path, launch for launch.
    -> {'loss', 'grad_norm', 'outputs'} as device tensors (no host sync)."""
    _check_mixup(mixup)
    pts = points if presampled else sample_points(points, npoints, subset=subset)
    if augment:
        pts = train_transforms(pts, draws=aug_draws)
    if mixup is not None:
        pts, targets = mixup.mix(pts, targets) if mixup_drawn else mixup(pts, targets)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        outputs = model(pts)
        loss = criterion(outputs.float(), targets.long())
    (loss / accum_iter).backward()
    gnorm = None
    if update and hasattr(optimizer, "flat_grad_views"):      # FlatAdamWEma: clip + AdamW in one pass (its own max_norm)
        gnorm = optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    elif update:
        params = [p for p in model.parameters() if p.grad is not None]
        if max_norm is not None:
            gnorm = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
    return {"loss": loss.detach(), "grad_norm": gnorm, "outputs": outputs.detach()}


class GraphedFinetuneStep:
    """The fine-tune iteration captured once as a hipGraph and replayed: at the reference's batch sizes (32-40 clouds) the
    step is a few hundred short launches and the host cannot keep the GPU fed.  Static inputs: the raw clouds, the
    labels and the random FPS subset (drawn on the host per call, copied in); the augmentation and DropPath/Dropout draws
    use the graph-safe device generator.  Needs an optimizer whose learning rates are device tensors that
    adjust_learning_rate fills in place: build_optimizer(..., capturable=True) or build_optimizer(..., flat=True).

    overlap_sampling=True: the point sampling (FPS 8192 -> point_all: one workgroup per cloud, 32-40 of the 256 CUs busy for
    >1 ms, a quarter of the step) is captured as its OWN graph and replayed on a second stream for the NEXT batch while the
    training graph of the current batch runs: call step(points, targets, next_points=<the following batch>).  Same
    arithmetic and the same order of host random draws as the single-graph form."""

    def __init__(self, model, criterion, optimizer, example_points, example_targets, npoints=1024, max_norm=None, bf16=True,
                 warmup_iters=3, rng=np.random, augment=True, overlap_sampling=False, mixup=None):
        """The `warmup_iters` un-captured iterations are real optimisation steps on the example batch (the allocator and
        the optimizer state must be warm before capture): pass warmup_iters=0 when the optimizer state already exists."""
        self.model, self.criterion, self.opt = model, criterion, optimizer
        self.npoints, self.max_norm, self.bf16, self.rng, self.augment = npoints, max_norm, bf16, rng, augment
        self.mixup, self._captured = _check_mixup(mixup), False
        self.point_all = min(POINT_ALL[npoints], example_points.size(1))
        self.points = example_points.clone()
        self.targets = example_targets.clone()
        self.subset = torch.zeros(npoints, dtype=torch.long, device=example_points.device)
        self._feed = streams.PinnedFeed(self.subset)
        self.overlap = bool(overlap_sampling)
        self._draw()
        self._draw_mixup()
        if self.overlap:
            self.pts = sample_points(self.points, npoints, subset=self.subset)
            self.staged = torch.zeros_like(self.pts)
            self.stage = streams.SideStage(example_points.device)
        streams.warm_up(self._body, warmup_iters)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with streams.capture(self.graph):
            self.out = self._body()
        self._captured = True
        if self.overlap:          # the sampler stream's graph: clouds + subset -> FPS + gather -> self.staged
            self.stage.capture(lambda: self.staged.copy_(sample_points(self.points, npoints, subset=self.subset)))
            torch.cuda.synchronize()

    def _draw(self):
        """Host draw of the shared FPS subset -> device, on the current stream."""
        self._feed.push([self.rng.choice(self.point_all, self.npoints, False).astype(np.int64)])

    def _draw_mixup(self):
        """Host draw of the mixup (lam, then the permutation) -> its device tensors and, once captured, the criterion's coefficients
        (before the capture the eager warm-up iterations stage them from the MixedTargets).  On the current stream, the replay's:
        unlike the subset this is never drawn one batch ahead, so the sequence of host draws stays subset, mixup, subset, mixup."""
        if self.mixup is None:
            return
        lam, _ = self.mixup.draw(self.points.size(0), self.points.device)
        stage = getattr(self.criterion, "stage", None)
        if self._captured and stage is not None:
            stage(lam)

    def _body(self):
        if self.overlap:
            return finetune_step(self.model, self.criterion, self.opt, self.pts, self.targets, npoints=self.npoints,
                                 max_norm=self.max_norm, bf16=self.bf16, augment=self.augment, presampled=True, mixup=self.mixup,
                                 mixup_drawn=True)
        return finetune_step(self.model, self.criterion, self.opt, self.points, self.targets, npoints=self.npoints,
                             max_norm=self.max_norm, bf16=self.bf16, subset=self.subset, augment=self.augment, mixup=self.mixup,
                             mixup_drawn=True)

    def __call__(self, points, targets, next_points=None):
        if not self.overlap:
            self.points.copy_(points, non_blocking=True)
            self.targets.copy_(targets, non_blocking=True)
            self._draw()
            self._draw_mixup()
            self.graph.replay()
            return self.out
        # the subset is drawn on the sampler stream, between the clouds' copy and the sampling graph that reads it
        self.stage.take(points, self.points, before_replay=self._draw)
        self.pts.copy_(self.staged)
        self.targets.copy_(targets, non_blocking=True)
        self._draw_mixup()
        if next_points is not None:               # queued BEFORE the training graph so that the two run side by side
            self.stage.enqueue(next_points, self.points, before_replay=self._draw)
        self.graph.replay()
        return self.out


def train_one_epoch(model, criterion, data_loader, optimizer, device, epoch, loss_scaler=None, max_norm=0,
                    mixup_fn=None, log_writer=None, args=None, npoints=0, print_freq=20, step=None):
    """Reference signature (P/engine_finetune.py:70-74).  The loss is read on the host every `print_freq` iterations
    (the reference syncs on loss.item() every iteration; a non-finite loss still stops the run at the next read).
    step: a GraphedFinetuneStep built on this model / optimizer -- the iteration is then a graph replay, and with
    overlap_sampling the loader is read one batch ahead so that the next batch's point sampling runs beside the current
    batch's training graph (accum_iter must be 1; a last batch of a different size runs eagerly).
    mixup_fn: None or a losses.PointMixup (TypeError otherwise), applied after train_transforms; with `step` it is the one the step
    was built with (a different one is a ValueError)."""
    _check_mixup(mixup_fn)
    step_mixup = getattr(step, "mixup", None)
    if mixup_fn is not None and step is not None and step_mixup is not mixup_fn:
        raise ValueError("mixup_fn must be the PointMixup the GraphedFinetuneStep was built with")
    mixup_fn = step_mixup if mixup_fn is None else mixup_fn
    model.train(True)
    accum_iter = getattr(args, "accum_iter", 1)
    if step is not None and accum_iter != 1:
        raise NotImplementedError("graph replay with gradient accumulation")
    optimizer.zero_grad(set_to_none=True)
    n_iter = len(data_loader)
    seen, loss_sum, last = 0, 0.0, None

    # (taxonomy, model_id, (points, label)) -> (points, targets) on the device, the next batch's while the current one trains
    loader = streams.LookAhead(data_loader, lambda item: tuple(t.to(device, non_blocking=True) for t in item[2][:2]))
    for it, (points, targets) in enumerate(loader):
        if it % accum_iter == 0:
            adjust_learning_rate(optimizer, it / n_iter + epoch, args)
        if step is not None and points.shape == step.points.shape:
            if step.overlap:
                nxt = None if loader.next is None else loader.next[0]
                out = step(points, targets, next_points=nxt if nxt is not None and nxt.shape == points.shape else None)
            else:
                out = step(points, targets)
        else:
            out = finetune_step(model, criterion, optimizer, points, targets, npoints=npoints,
                                max_norm=max_norm if max_norm else None, bf16=getattr(args, "bf16", True),
                                update=(it + 1) % accum_iter == 0, accum_iter=accum_iter, mixup=mixup_fn)
        last = out["loss"]
        if (it + 1) % print_freq == 0 or it + 1 == n_iter:
            v = float(last)
            if not math.isfinite(v):
                print("Loss is {}, stopping training".format(v))
                sys.exit(1)
            loss_sum += v
            seen += 1
            if log_writer is not None:
                log_writer.add_scalar("loss", v, int((it / n_iter + epoch) * 1000))
    lrs = [float(g["lr"]) for g in optimizer.param_groups]
    return {"loss": loss_sum / max(seen, 1), "lr": max(lrs)}


@torch.no_grad()
def evaluate(data_loader, model, device, npoints=1024, bf16=True):
    """Top-1 accuracy / mean cross-entropy over a loader of (.., .., (points, label)) batches; test clouds are reduced
    to `npoints` by FPS alone (P/main_finetune.py validate: misc.fps(points, npoints))."""
    criterion = torch.nn.CrossEntropyLoss(reduction="sum")
    model.eval()
    n, correct, loss = 0, 0, 0.0
    for batch in data_loader:
        data = batch[-1]
        points, target = data[0].to(device), data[1].to(device).long().view(-1)
        if points.size(1) != npoints:
            points = ops.fps(points.contiguous(), npoints)[1]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            logits = model(points).float()
        loss += float(criterion(logits, target))
        correct += int((logits.argmax(-1) == target).sum())
        n += target.numel()
    return {"acc1": 100.0 * correct / max(n, 1), "loss": loss / max(n, 1), "n": n}


# --------------------------------------------------------------------------- voting evaluation
# P/tools/runner_finetune.py:271-335 (validate_vote) and :399-461 (test_vote): per batch one FPS to point_all, then `times` votes,
# each a host-drawn subset of the FPS order shared by the batch, the test transform PointcloudScaleAndTranslate drawn per cloud,
# and an eval forward; the mean of the vote logits decides.  Here the host makes exactly the reference's np.random calls, in its
# order, before anything is launched; then ONE launch builds all V*B vote clouds, ONE forward runs them (split into chunks of
# `max_clouds`), and ONE launch computes the head of every vote, the vote mean, the argmax and the correct count.  That last
# launch pools the tokens the way the model does (vote_tail): PointTransformer [cls ; max] (ops.cls_tail_vote), the Point-M2AE
# classifiers mean + max or [mean ; max] (ops.cls_tail_vote_pool).

DEFAULT_VOTE_MAX_CLOUDS = 512     # clouds per forward_tokens call: B=32 x 10 votes fits in one


def _check_npoints(npoints):
    if npoints not in POINT_ALL:
        raise NotImplementedError("npoints %d" % npoints)


def vote_point_all(npoints, n0):
    """point_all of the vote sampling (P/tools/runner_finetune.py:284-294): POINT_ALL[npoints], capped at the cloud size."""
    _check_npoints(npoints)
    return min(POINT_ALL[npoints], n0)


def vote_tail(model):
    """The one-launch eval head + vote mean for `model`'s pooling -> fn(x, labels, V, correct, votes=None) -> (mean, pred):
    PointTransformer -> ops.cls_tail_vote ([x[:, 0] ; max]); a Point-M2AE classifier -> ops.cls_tail_vote_pool with
    POOL_MODES[model.pool].  Any other model raises TypeError: a tail that pools differently from the model must not run."""
    from .point_m2ae_cls import POOL_MODES, PointM2AEClassifier
    from .point_transformer import PointTransformer
    head = getattr(model, "cls_head_finetune", None)
    if isinstance(model, PointTransformer):
        return lambda x, labels, V, correct, votes=None: ops.cls_tail_vote(x, head, labels, V, correct, votes=votes)
    if isinstance(model, PointM2AEClassifier):
        mode = POOL_MODES[model.pool]
        return lambda x, labels, V, correct, votes=None: ops.cls_tail_vote_pool(x, head, mode, labels, V, correct, votes=votes)
    raise TypeError("voting evaluation supports PointTransformer and the Point-M2AE classifiers, not %s" % type(model).__name__)


def draw_votes(rng, point_all, npoints, times, B):
    """The host draws of one batch, in the reference's order: per vote np.random.choice(point_all, npoints, False)
    (runner_finetune.py:294), then per cloud uniform(2/3, 3/2, 3) and uniform(-0.2, 0.2, 3) (test_transforms =
    PointcloudScaleAndTranslate, datasets/data_transforms.py:31-32), cast to f32 like torch.from_numpy(...).float().
    -> subsets (V,npoints) int64, scale (V,B,3) f32, shift (V,B,3) f32 (numpy)."""
    subsets = np.empty((times, npoints), dtype=np.int64)
    scale = np.empty((times, B, 3), dtype=np.float32)
    shift = np.empty((times, B, 3), dtype=np.float32)
    for v in range(times):
        subsets[v] = rng.choice(point_all, npoints, False)
        for b in range(B):
            scale[v, b] = rng.uniform(low=2. / 3., high=3. / 2., size=[3])
            shift[v, b] = rng.uniform(low=-0.2, high=0.2, size=[3])
    return subsets, scale, shift


class _VoteDraws:
    """Device copies of one batch's draws, staged through a streams.PinnedFeed (asynchronous copies, like the fine-tune step's
    subset).  Before the first stage() they hold a draw-free warm-up value (identity transform)."""

    def __init__(self, times, npoints, B, device):
        self.times, self.npoints, self.B = times, npoints, B
        self.subsets = torch.arange(npoints, dtype=torch.long, device=device).repeat(times, 1)
        self.scale = torch.ones(times, B, 3, dtype=torch.float32, device=device)
        self.shift = torch.zeros(times, B, 3, dtype=torch.float32, device=device)
        self._feed = streams.PinnedFeed(self.subsets, self.scale, self.shift)

    def stage(self, rng, point_all):
        self._feed.push(draw_votes(rng, point_all, self.npoints, self.times, self.B))


def vote_batch(model, points, labels, subsets, scale, shift, point_all, correct, bf16=True, max_clouds=None, votes=None):
    """The votes of one batch on the device, no host sync: FPS (B,N0,3) -> point_all, vote_sample -> (V*B,npoints,3),
    forward_tokens in chunks of `max_clouds` clouds, the model's vote tail (vote_tail; TypeError before any launch for a model it
    does not know).  The model must be in eval mode (callers: validate_vote, GraphedVoteEval).  correct: int64 device counter
    (+= correct predictions).  -> (mean logits (B,cls_dim), pred (B,))."""
    tail = vote_tail(model)
    V = subsets.size(0)
    fps_idx = ops.furthest_point_sample(points, point_all)
    pts = ops.vote_sample(points, fps_idx, subsets, scale, shift)
    chunk = max_clouds or DEFAULT_VOTE_MAX_CLOUDS
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        if pts.size(0) <= chunk:
            x = model.forward_tokens(pts)
        else:
            x = torch.cat([model.forward_tokens(pts[i:i + chunk]) for i in range(0, pts.size(0), chunk)], dim=0)
    return tail(x.contiguous(), labels, V, correct, votes=votes)


class GraphedVoteEval:
    """The votes of one batch shape captured once as a hipGraph: FPS -> vote_sample -> forward_tokens over V*B clouds ->
    the model's vote tail.  Static inputs: points, labels, subsets, scale and shift (the draws are made on the host per call and copied
    in); outputs `mean` (B,cls_dim), `pred` (B,), `votes` (V,B,cls_dim) when keep_votes, and the running int64 count `correct`.
    A call copies, stages the draws and replays: no host sync.

    The graph reads the parameters, BatchNorm running statistics and bf16 weight copies where they live, so it stays valid while
    training continues in place between calls (a flat optimizer rewrites the weights and their bf16 shadows in place).  Should
    the parameters be re-pointed to new storage (an optimizer that flattens them built after this object), the next call
    captures again."""

    def __init__(self, model, example_points, example_labels, npoints=1024, times=10, bf16=True, rng=np.random, max_clouds=None,
                 keep_votes=False):
        self.model = model.module if hasattr(model, "module") else model
        B, N0 = example_points.shape[:2]
        self.npoints, self.times, self.bf16, self.rng, self.max_clouds = npoints, times, bf16, rng, max_clouds
        self.point_all = vote_point_all(npoints, N0)
        vote_tail(self.model)
        dev = example_points.device
        self.points = example_points.detach().float().contiguous().clone()
        self.labels = example_labels.detach().reshape(-1).to(dev, torch.long).clone()
        self.draws = _VoteDraws(times, npoints, B, dev)
        self.correct = torch.zeros(1, dtype=torch.long, device=dev)
        self.votes = torch.zeros(times, B, self.model.cls_dim, dtype=torch.float32, device=dev) if keep_votes else None
        self._capture()

    def _storage(self):
        return tuple(t.data_ptr() for t in list(self.model.parameters()) + list(self.model.buffers()))

    def _body(self, correct):
        d = self.draws
        return vote_batch(self.model, self.points, self.labels, d.subsets, d.scale, d.shift, self.point_all, correct,
                          bf16=self.bf16, max_clouds=self.max_clouds, votes=self.votes)

    @torch.no_grad()
    def _capture(self):
        was = self.model.training
        self.model.eval()
        try:
            streams.warm_up(lambda: self._body(torch.zeros(1, dtype=torch.long, device=self.points.device)), 1)    # its own counter
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with streams.capture(self.graph):
                self.mean, self.pred = self._body(self.correct)
            torch.cuda.synchronize()
        finally:
            self.model.train(was)
        self._captured = self._storage()

    def __call__(self, points, labels, rng=None):
        """rng: the host generator of this call's draws (default: the one given at construction)."""
        if self._storage() != self._captured:
            self._capture()
        self.points.copy_(points, non_blocking=True)
        self.labels.copy_(labels.reshape(-1), non_blocking=True)
        self.draws.stage(self.rng if rng is None else rng, self.point_all)
        self.graph.replay()
        return self.mean, self.pred


@torch.no_grad()
def validate_vote(model, data_loader, device, npoints=1024, times=10, bf16=True, rng=np.random, graphed=True, max_clouds=None,
                  outputs=False):
    """Voting accuracy over a loader of (.., .., (points, label)) batches (P/tools/runner_finetune.py:271-335), with the same
    np.random calls in the same order as the reference: seeded alike, both use the same subsets and transforms.
    graphed: True -> a GraphedVoteEval is captured on the first batch and replayed for every batch of that shape (a ragged
    last batch runs eagerly through the same kernels); a GraphedVoteEval instance is reused (its capture outlives the call; the
    draws still come from `rng`);
    False -> eager.  max_clouds: clouds per forward (default DEFAULT_VOTE_MAX_CLOUDS = 512; the V*B forward is split above).
    One host sync per call, at the end.  Predictions and labels are gathered across ranks like the reference.
    -> {"acc_vote", "n"}; outputs=True adds the local "pred" (n,), "mean" (n,cls_dim) and "votes" (V,n,cls_dim)."""
    raw = model.module if hasattr(model, "module") else model
    _check_npoints(npoints)
    vote_tail(raw)
    was = raw.training
    raw.eval()
    try:
        g = graphed if isinstance(graphed, GraphedVoteEval) else None
        if g is not None and outputs and g.votes is None:
            raise ValueError("outputs=True needs a GraphedVoteEval built with keep_votes=True")
        counter = None
        eager_draws = {}
        preds, labels, means, votes = [], [], [], []
        for batch in data_loader:
            data = batch[-1]
            points = data[0].to(device, non_blocking=True).float().contiguous()
            label = data[1].to(device, non_blocking=True).long().reshape(-1)
            if g is None and graphed is True:
                g = GraphedVoteEval(raw, points, label, npoints=npoints, times=times, bf16=bf16, rng=rng, max_clouds=max_clouds,
                                    keep_votes=outputs)
            if counter is None:
                counter = g.correct if g is not None else torch.zeros(1, dtype=torch.long, device=device)
                counter.zero_()
            if g is not None and points.shape == g.points.shape:
                mean, pred = g(points, label, rng=rng)
                mean, pred = mean.clone(), pred.clone()
                vt = g.votes.clone() if outputs else None
            else:
                B = points.size(0)
                point_all = vote_point_all(npoints, points.size(1))
                d = eager_draws.get(B)
                if d is None:
                    d = eager_draws[B] = _VoteDraws(times, npoints, B, points.device)
                d.stage(rng, point_all)
                vt = torch.empty(times, B, raw.cls_dim, dtype=torch.float32, device=points.device) if outputs else None
                mean, pred = vote_batch(raw, points, label, d.subsets, d.scale, d.shift, point_all, counter, bf16=bf16,
                                        max_clouds=max_clouds, votes=vt)
            preds.append(pred)
            labels.append(label)
            if outputs:
                means.append(mean)
                votes.append(vt)
    finally:
        raw.train(was)
    if not preds:
        return {"acc_vote": 0.0, "n": 0}
    pred, label = torch.cat(preds), torch.cat(labels)
    from .validate import gather_tensor
    import torch.distributed as dist
    if dist.is_initialized() and dist.get_world_size() > 1:
        gp, gl = gather_tensor(pred), gather_tensor(label)
        correct, n = int((gp == gl).sum()), gl.numel()
    else:
        correct, n = int(counter), label.numel()
    # the reference's arithmetic: (pred == label).sum() / float(n) * 100. in float32
    acc = float(torch.tensor(correct) / float(n) * 100.)
    out = {"acc_vote": acc, "n": n}
    if outputs:
        out.update(pred=pred, mean=torch.cat(means), votes=torch.cat(votes, dim=1))
    return out


def test_vote(model, data_loader, device, npoints=1024, times=10, bf16=True, rng=np.random, graphed=True, max_clouds=None):
    """P/tools/runner_finetune.py:399-461: the same voting pass as validate_vote; returns the accuracy."""
    return validate_vote(model, data_loader, device, npoints=npoints, times=times, bf16=bf16, rng=rng, graphed=graphed,
                         max_clouds=max_clouds)["acc_vote"]

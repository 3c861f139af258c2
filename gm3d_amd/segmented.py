"""The data-parallel pretrain step shared by both pretraining models: the backward cut into NSEG segments, each segment's gradient
all-reduce issued eagerly behind it (so that it runs beside the next segment's backward), then clip + AdamW + EMA.  Replayed as
NSEG + 1 hipGraphs with the collectives between them -- no collective is captured.

SegmentedStep owns the process group, the flat-buffer bookkeeping, the collectives, the capture chain and the replay loop; a model's
step (engine_pretrain.SegmentedDDPStep, point_m2ae.SegmentedM2AEStep) says where its backward is cut.  The broadcasts and the update
half that every step of the package shares live here as well, so that no model module has to import another for them."""
import torch
import torch.distributed as dist

from . import streams


def _broadcast_tensors(tensors, src=0, group=None):
    """Coalesced broadcast: one collective per dtype (pack, broadcast, unpack)."""
    by_dtype = {}
    for t in tensors:
        by_dtype.setdefault(t.dtype, []).append(t)
    with torch.no_grad():
        for ts in by_dtype.values():
            flat = torch.cat([t.reshape(-1) for t in ts])
            dist.broadcast(flat, src=src, group=group)
            off = 0
            for t in ts:
                t.copy_(flat[off:off + t.numel()].view_as(t))
                off += t.numel()


def broadcast_state(model=None, model_ema=None, optimizer=None, src=0, group=None):
    """What the DDP constructor does at P/main_pretrain_multi_gpu.py:309-311, extended to everything a rank keeps: rank `src`'s
    student parameters and buffers (integer counters included), EMA teacher and -- for FlatAdamWEma -- the flat master / moment
    buffers and the step counter overwrite the other ranks'; the bf16 GEMM shadows are re-derived.  No-op without a group of >1."""
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    ts = []
    flat = optimizer is not None and hasattr(optimizer, "flat_grad_views")
    if flat:
        ts += [optimizer.P, optimizer.M, optimizer.V, optimizer.step_dev]
        if optimizer.E is not None:
            ts.append(optimizer.E)
    seen = {t.data_ptr() for t in ts}
    lo, hi = (optimizer.P.data_ptr(), optimizer.P.data_ptr() + optimizer.P.numel() * 4) if flat else (0, 0)
    elo, ehi = (optimizer.E.data_ptr(), optimizer.E.data_ptr() + optimizer.E.numel() * 4) if flat and optimizer.E is not None else (0, 0)
    for mod in (model.module if hasattr(model, "module") else model, getattr(model_ema, "ema", model_ema)):
        if mod is None:
            continue
        for t in list(mod.parameters()) + list(mod.buffers()):
            a = t.data_ptr()
            if a in seen or lo <= a < hi or elo <= a < ehi:       # views of the flat buffers travel with them
                continue
            seen.add(a)
            ts.append(t.data)
    _broadcast_tensors(ts, src=src, group=group)
    if flat:
        optimizer.sync_shadows()


def broadcast_buffers(model, src=0, group=None):
    """DDP's default broadcast_buffers=True: rank 0's BatchNorm running statistics overwrite the other
    ranks' before the forward pass; one coalesced collective (3 launches: pack, broadcast, unpack)."""
    bufs = [b for b in model.buffers() if b.dtype.is_floating_point]
    if not bufs or not dist.is_initialized() or dist.get_world_size(group) == 1:
        return
    flat = torch.cat([b.reshape(-1) for b in bufs])
    dist.broadcast(flat, src=src, group=group)
    views, off = [], 0
    for b in bufs:
        views.append(flat[off:off + b.numel()].view_as(b))
        off += b.numel()
    with torch.no_grad():
        torch._foreach_copy_(bufs, views)


def step_update(model, model_ema, optimizer, clip_grad=5.0):
    """Second half (P/util/misc.py:262-266 + P/engine_pretrain.py:208-212): clip -> AdamW -> EMA."""
    raw = model.module if hasattr(model, "module") else model
    if hasattr(optimizer, "flat_grad_views"):      # FlatAdamWEma: clip + AdamW + EMA(params) + bf16 shadows, one pass
        grad_norm = optimizer.step()
        if model_ema is not None:                  # (plain Point-MAE pre-training has no teacher)
            model_ema.update(raw)                  # BatchNorm buffers only
        return grad_norm
    grad_norm = torch.nn.utils.clip_grad_norm_(raw.parameters(), clip_grad, foreach=True)
    optimizer.step()
    model_ema.update(raw)
    return grad_norm


class SegmentedStep:
    """What a segmented data-parallel step is apart from its model.  A subclass sets NSEG and implements

        _segment(k, first_input=None)   segment k's backward, its gradients put into their flat slots with _store(k, grads);
                                        segment 0 runs the forward on `first_input` first and returns the step's output dict

    and its own _eager / __call__ entries (the models take different inputs), which run the segments through _run.  Needs
    FlatAdamWEma built with segment_of=: each segment's weight gradients are one contiguous range of the flat buffer.
    args.accum_iter > 1: the segments' gradients are summed over the window in a second flat buffer and the collectives run once,
    on the sums, after the window's last backward (no overlap in that mode)."""

    NSEG = None

    def __init__(self, model, model_ema, optimizer, args, epoch, process_group=None, broadcast=True):
        self.model, self.ema, self.opt, self.args, self.epoch = model, model_ema, optimizer, args, epoch
        self.raw = model.module if hasattr(model, "module") else model
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # RCCL averages inside its ring kernel (ReduceOp.AVG).  A group of ONE rank keeps SUM: AVG there runs RCCL's one-rank
        # pre-multiply kernel over the whole range (71 us per collective measured, 0.21 ms per step: tools/seg_timeline.py), which
        # no N > 1 run executes -- a one-rank rehearsal of the layout should not be charged for it.
        self._avg = dist.is_initialized() and dist.get_backend(process_group) == "nccl" and self.world > 1
        self.accum = getattr(args, "accum_iter", 1)
        if broadcast:
            broadcast_state(self.raw, model_ema, optimizer, group=process_group)
        views = dict((id(p), g) for p, g in optimizer.flat_grad_views())
        self.seg_params = {sg: list(ps) for sg, ps in optimizer.segment_params.items()}
        self.seg_views = {sg: [views[id(p)] for p in ps] for sg, ps in self.seg_params.items()}
        self.graphs = None

    def _capture(self, first_input):
        """NSEG + 1 graphs in one memory pool: a graph per segment (segment 0's returns the output dict), then clip + AdamW + EMA."""
        self.graphs = [torch.cuda.CUDAGraph() for _ in range(self.NSEG + 1)]
        with streams.capture(self.graphs[0]):
            self.out = self._segment(0, first_input)
        for k in range(1, self.NSEG):
            with streams.capture(self.graphs[k], pool=self.graphs[0].pool()):
                self._segment(k)
        with streams.capture(self.graphs[self.NSEG], pool=self.graphs[0].pool()):
            self.out["grad_norm"] = self._update()

    def _store(self, seg, grads):
        """gradients of one segment -> their slots of the flat buffer (ONE multi-tensor copy; unused parameters: zeros)."""
        views, have, zero = self.seg_views[seg], [], []
        for v, g in zip(views, grads):
            if g is not None and g.data_ptr() == v.data_ptr():
                continue                      # written into its slot by the backward node itself (gemm.wgrad)
            (have if g is not None else zero).append((v, g))
        if have:
            torch._foreach_copy_([v for v, _ in have], [g for _, g in have])
        if zero:
            torch._foreach_zero_([v for v, _ in zero])

    def _update(self):
        self.opt.mark_grads_filled()        # every segment stored its gradients into G: step() must not gather from p.grad
        return step_update(self.model, self.ema, self.opt)

    def _reduce(self, seg):
        """async all-reduce (mean) of one segment's range of the flat gradient buffer on the process group's stream."""
        if not dist.is_initialized():
            return None
        lo, hi = self.opt.segment_ranges[seg]
        buf = self.opt.G[lo:hi]
        w = dist.all_reduce(buf, op=dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM, group=self.group, async_op=True)
        return (w, buf)

    def _wait(self, works):
        for item in works:
            if item is None:
                continue
            w, buf = item
            w.wait()
            if not self._avg and self.world > 1:
                buf.div_(self.world)

    def _run(self, phases, update=True):
        """phases: NSEG callables (graph replays or the eager segments).  accum_iter == 1: each segment's collective is issued
        right behind its phase; accum_iter > 1: gradients join the window's sum, collectives only when `update`.
        -> whether the gradients are complete (the update may run)."""
        if self.accum == 1:
            works = []
            for k in range(self.NSEG):
                phases[k]()
                works.append(self._reduce(k))
            self._wait(works)
            return True
        for k in range(self.NSEG):
            phases[k]()
        self.opt.accumulate(last=update)
        if update:
            self._wait([self._reduce(k) for k in range(self.NSEG)])
        return update

    def _replay(self, update=True):
        """the captured step on the inputs its caller has staged.  update=False (gradient accumulation, not the last micro-batch
        of its window): no update graph; the returned grad_norm is None."""
        if self._run([g.replay for g in self.graphs[:self.NSEG]], update):
            self.graphs[self.NSEG].replay()
            return self.out
        out = dict(self.out)
        out["grad_norm"] = None
        return out

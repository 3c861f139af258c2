"""When and on which stream every weight gradient dW = dy^T @ x of a backward runs (gemm.route_wgrad / multi_splits decide on what).

    with async_wgrad(device): <backward>    the region (the engines' backward)
    stack(jobs, takes_part)                 the four stacked products of a block stack, at the end of its backward
    defer_wgrad(dy, x, w)                   one layer outside the stacks (heads, positional MLPs, token embeds)
    Batch                                   the products of ONE backward node (EmbedFn), launched together at its end

Inside a region the deep stack's four go to a side stream at once (what follows them in the backward is the mini-PointNet's HBM-bound
passes, which leave the matrix cores idle); the shallow decoders' are DEFERRED to that point (beside the encoder's latency-bound
input-gradient chain, which comes right after them, they cost 3.7 %): their destinations are slots of the flat gradient buffer, filled
later.  The exit runs what is still deferred and joins.  Outside a region everything runs in line.  DESIGN.md 3b' has the invariants."""
import torch

from . import gemm, optim, streams

ASYNC_WGRAD = True        # (tests flip it)
WGRAD_MIN_BLOCKS = 5      # stacks with fewer blocks (the 4-block decoders) DEFER their weight-gradient GEMMs to the deep stack's fork point
DEFER_HEAD_WGRAD = False  # the heads' / positional MLP's weight gradients inside the stacks' one-launch form (defer_wgrad): measured
#                           0.4 % slower (7.43 vs 7.39 ms same-box): three small products are cheaper where they stand than as extra tiles there
_side = {}                # (device type, index) -> the regions' side stream


class _Region:
    """stream: the side stream while a region is active; used: a stack forked to it; deferred: [(tensors to keep alive, requests)]"""
    def __init__(self):
        self.stream, self.used, self.min_blocks, self.defer_heads, self.deferred = None, False, WGRAD_MIN_BLOCKS, False, []


region = _Region()


def current():
    """the active region, or None"""
    return region if region.stream is not None else None


def _many(reqs):
    """[(dy, x, out slot | None), ...] -> [dW, ...]: one launch for all of them where the NT kernel takes every request
    (gemm.wgrad_nt_multi), else one batched GEMM per request."""
    if gemm.MULTI_WGRAD and len(reqs) > 1 and all(gemm.wgrad_multi_ok(dy, x, out) for dy, x, out in reqs):
        res = []                      # the kernel takes 16 problems per launch: ceil(n / 16) launches of about equal size
        per = -(-len(reqs) // -(-len(reqs) // 16))
        for i in range(0, len(reqs), per):
            chunk = reqs[i:i + per]
            res += gemm.wgrad_nt_multi(chunk) if len(chunk) > 1 else [gemm.wgrad(*chunk[0])]
        return res
    return [gemm.wgrad(dy, x, out) for dy, x, out in reqs]


def _with_deferred(own=()):
    """the deferred requests, plus `own` (the calling stack's), on the current stream -> the results of `own`"""
    jobs, region.deferred = region.deferred, []
    cur = torch.cuda.current_stream()
    reqs = []
    for tensors, rq in jobs:
        for t in tensors:
            t.record_stream(cur)
        reqs += rq
    res = _many(reqs + list(own)) if (reqs or own) else []
    return res[len(reqs):]


def stack(jobs, takes_part):
    """jobs: [(dy (nblk,R,N), x (nblk,R,K), the nblk parameters), ...] in the order fc2, fc1, proj, qkv -> the four dW (nblk,N,K),
    written straight into the parameters' slots of the optimizer's flat gradient buffer when the same-kind weights of the stack are
    adjacent there (optim._kind_key) and hold no gradient yet (the slot is overwritten): autograd adopts the slot views as .grad.
    takes_part: inside a region the stack forks or defers (TransformerStackFn); MaskedStackFn stays out: now, on the current stream."""
    cuda, nblk = jobs[0][0].is_cuda, jobs[0][0].shape[0]
    unset = [cuda and all(p.grad is None for p in ps) for _, _, ps in jobs]      # per kind: no gradient accumulated yet
    fresh = all(unset)
    # two slot policies: a stack that takes part takes slots only when all four kinds are unset, one that stays out kind by kind
    slots = [optim.grad_slots.stacked(ps) if ok and (fresh or not takes_part) else None for ok, (_, _, ps) in zip(unset, jobs)]
    own = [(dy, x, sl) for (dy, x, _), sl in zip(jobs, slots)]
    ws = region.stream if takes_part and fresh else None
    if ws is None or (nblk < region.min_blocks and any(sl is None for sl in slots)):
        return _many(own)
    keep = [t for dy, x, _ in jobs for t in (dy, x)]
    if nblk < region.min_blocks:
        region.deferred.append((keep, own))
        return slots
    streams.fork(ws, who="wgrads.stack: weight-gradient stream (async_wgrad region)")
    region.used = True
    for t in keep:
        t.record_stream(ws)
    with torch.cuda.stream(ws):     # the deferred decoders' requests and this stack's own: ONE launch (+ one slab sum) where the kernel takes them all
        return _with_deferred(own)


def defer_wgrad(dy, x, w=None):
    """dW (N,K) f32 = dy (R,N)^T @ x (R,K) for a layer OUTSIDE the block stacks (heads, positional MLP), w its weight parameter.
    Inside the engine's backward region, when w has a slot in the optimizer's flat gradient buffer and no gradient yet (nothing will
    read or add to the result before the region ends), the product joins the stacks' one-launch weight gradients and lands in the slot;
    elsewhere, or when the kernel does not take the shape, it is computed now."""
    if (region.stream is not None and gemm.MULTI_WGRAD and (DEFER_HEAD_WGRAD or region.defer_heads) and w is not None and w.is_leaf
            and w.grad is None and dy.dim() == 2 and dy.is_contiguous() and x.is_contiguous()):
        slot = optim.grad_slots.get(w) if optim.ENABLE_DIRECT_WGRAD else None
        if slot is not None and slot.is_contiguous() and slot.numel() == dy.shape[1] * x.shape[1]:
            out = slot.view(1, dy.shape[1], x.shape[1])
            if gemm.wgrad_multi_ok(dy.unsqueeze(0), x.unsqueeze(0), out):
                region.deferred.append(((dy, x), [(dy.unsqueeze(0), x.unsqueeze(0), out)]))
                return out[0]
    return gemm.wgrad(dy, x)


class Batch:
    """The weight-gradient products of ONE backward node: ONE launch at its end (gemm.wgrad_nt_multi: together they fill the chip with
    row splits in proportion to their rows) instead of launches that each cut themselves into 64 slabs.  add(dy (R,N), x (R,K)) ->
    dW (N,K) f32, filled by flush() at the latest; a request the NT kernel does not take runs at once, a single one on its own splits."""
    def __init__(self, adt):
        self.multi, self.reqs = gemm.MULTI_WGRAD and adt == torch.bfloat16 and gemm.ENABLED, []

    def add(self, dy, x):
        if self.multi and dy.is_contiguous() and x.is_contiguous() and gemm.wgrad_multi_ok(dy.unsqueeze(0), x.unsqueeze(0), None):
            out = torch.empty(1, dy.shape[1], x.shape[1], dtype=torch.float32, device=dy.device)
            self.reqs.append((dy.unsqueeze(0), x.unsqueeze(0), out))
            return out[0]
        return gemm.wgrad(dy, x)

    def flush(self):
        if len(self.reqs) > 1:
            gemm.wgrad_nt_multi(self.reqs)
        elif self.reqs:
            gemm.wgrad_nt(*self.reqs[0])


class async_wgrad:
    """with async_wgrad(device): <backward>  -- weight-gradient GEMMs of the deep block stacks run on a side stream during the
    region; on exit the current stream waits for it (so whatever follows -- gradient gather, all-reduce, optimizer -- sees them).
    defer_heads: weight gradients of layers outside the block stacks (defer_wgrad: token embeds, heads, positional MLPs) join ONE launch
    at the region's exit -- for a model with many small such layers (Point-M2AE: 19) that is 2 launches instead of 38; for the
    north-star model's three it measured slower (DEFER_HEAD_WGRAD)."""
    def __init__(self, device, min_blocks=None, defer_heads=False):
        self.dev, self.min_blocks = torch.device(device), (WGRAD_MIN_BLOCKS if min_blocks is None else min_blocks)
        self.defer_heads = bool(defer_heads)

    def __enter__(self):
        if ASYNC_WGRAD and self.dev.type == "cuda":
            key = (self.dev.type, self.dev.index)
            if key not in _side:
                _side[key] = torch.cuda.Stream(device=self.dev)
            region.stream, region.used, region.min_blocks, region.defer_heads = _side[key], False, self.min_blocks, self.defer_heads
            if self.defer_heads:
                gemm.prepare_transposes()       # the small layers' transposed weight shadows: one launch per eight, not one per layer
        return self

    def __exit__(self, *exc):
        ws, used = region.stream, region.used
        if region.defer_heads:
            gemm.drop_transposes()
        region.stream, region.used, region.defer_heads = None, False, False
        if region.deferred:                 # no deep stack came by to take them along: run them here, in line
            if exc[0] is None:
                _with_deferred()
            region.deferred = []
        if ws is not None and used:
            streams.join(ws)
        return False

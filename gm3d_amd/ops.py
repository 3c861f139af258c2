"""Torch-facing operators over the C ABI (include/gm3d.h).

Names, argument meaning and error behaviour mirror the reference-side interfaces the
GM3D pretrain path imports:
  furthest_point_sample / gather_operation <- pointnet2_ops.pointnet2_utils
      (Point-MAE_SA3D/models_mae_learn_loss.py:931-932, utils/miscc.py:18-19)
  KNN                                       <- knn_cuda.KNN (models_mae_learn_loss.py:924,946)
  ChamferDistanceL2 / ChamferDistanceL1     <- extensions.chamfer_dist (models_mae_learn_loss.py:188,407)
plus two fused entry points the reference has no counterpart for (knn_group, attention).
PyTorch is plumbing only here: it owns device memory and the current HIP stream.
"""
import ctypes

import torch

from . import _capi
from ._capi import check, lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer:
    """Optional per-launch timing with HIP events recorded on the stream the kernels are launched on
    (torch's current stream).  bench.py installs one over its timed region for the roofline figures;
    when none is installed the wrappers add nothing.  `only` restricts timing to some kernel names."""

    def __init__(self, only=None):
        self.only = set(only) if only else None
        self.records = {}   # name -> [(start_event, end_event, meta)]

    def wants(self, name):
        return self.only is None or name in self.only

    @staticmethod
    def bracket_overhead_ms(n=200):
        """Median elapsed time of an EMPTY event bracket on the current stream: what start/stop recording itself adds to
        every measured launch (subtract it before comparing with rocprof's kernel durations)."""
        ev = []
        for _ in range(n):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); e.record()
            ev.append((s, e))
        torch.cuda.synchronize()
        ms = sorted(s.elapsed_time(e) for s, e in ev)
        return ms[len(ms) // 2]

    def summary(self):
        """name -> {"launches", "avg_ms", "total_ms", "meta"} (synchronises)."""
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = [s.elapsed_time(e) for s, e, _ in recs]
            out[name] = {"launches": len(ms), "avg_ms": sum(ms) / len(ms), "total_ms": sum(ms), "meta": recs[0][2],
                         "per_launch": [(m, r[2]) for m, r in zip(ms, recs)]}
        return out


_timer = None


def set_kernel_timer(timer):
    global _timer
    _timer = timer


def _launch(name, meta, fn, *args):
    """Call one C-ABI entry point, check its status, optionally bracket it with HIP events."""
    t = _timer
    if t is None or not t.wants(name):
        check(fn(*args), name)
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    check(fn(*args), name)
    e.record()
    t.records.setdefault(name, []).append((s, e, meta))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _require(t, dtype, name, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must be a GPU tensor (gm3d_amd has no CPU fallback)" % name)
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)


# ------------------------------------------------------------------ FPS / gather
def fps(xyz, npoint, return_centers=True):
    """xyz (B,N,3) f32 contiguous -> (idx (B,npoint) int32, centers (B,npoint,3) f32 | None)."""
    _require(xyz, torch.float32, "xyz")
    if xyz.dim() != 3 or xyz.size(2) != 3:
        raise RuntimeError("xyz must be (B,N,3)")
    B, N, _ = xyz.shape
    idx = torch.empty(B, npoint, dtype=torch.int32, device=xyz.device)
    cen = torch.empty(B, npoint, 3, dtype=torch.float32, device=xyz.device) if return_centers else None
    _launch("gm3d_fps", {"B": B, "N": N, "npoint": int(npoint)}, lib.gm3d_fps, _ptr(xyz), B, N, int(npoint), _ptr(idx), _ptr(cen), _stream())
    return idx, cen


def furthest_point_sample(xyz, npoint):
    """pointnet2_utils.furthest_point_sample: (B,N,3) f32 -> (B,npoint) int32, non-differentiable."""
    with torch.no_grad():
        return fps(xyz.detach(), npoint, return_centers=False)[0]


class _GatherOperation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _require(features, torch.float32, "features")
        _require(idx, torch.int32, "idx")
        B, C, N = features.shape
        M = idx.size(1)
        out = torch.empty(B, C, M, dtype=torch.float32, device=features.device)
        _launch("gm3d_gather_points", {"B": B, "C": C, "N": N, "M": M}, lib.gm3d_gather_points, _ptr(features), _ptr(idx), B, C, N, M, _ptr(out), _stream())
        ctx.save_for_backward(idx)
        ctx.N = N
        ctx.mark_non_differentiable(idx)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        g = grad_out.contiguous().float()
        B, C, M = g.shape
        gf = torch.empty(B, C, ctx.N, dtype=torch.float32, device=g.device)
        _launch("gm3d_gather_points_grad", {"B": B, "C": C, "N": ctx.N, "M": M}, lib.gm3d_gather_points_grad, _ptr(g), _ptr(idx), B, C, ctx.N, M, _ptr(gf), _stream())
        return gf, None


def gather_operation(features, idx):
    """pointnet2_utils.gather_operation: features (B,C,N) f32, idx (B,M) int32 -> (B,C,M)."""
    return _GatherOperation.apply(features, idx)


# ------------------------------------------------------------------ voting evaluation (tools/runner_finetune.py:271-335)
def vote_sample(points, fps_idx, subsets, scale, shift, out=None):
    """All vote clouds of a batch in one launch: points (B,N0,3) f32, fps_idx (B,point_all) int32, subsets (V,npoints) int64,
    scale / shift (V,B,3) f32 -> (V*B,npoints,3) f32, row v*B+b = points[b][fps_idx[b][subsets[v]]] * scale[v,b] + shift[v,b]
    (bit-equal to index_select + gather_operation + the reference's `pc*xyz1 + xyz2`)."""
    _require(points, torch.float32, "points")
    _require(fps_idx, torch.int32, "fps_idx")
    _require(subsets, torch.int64, "subsets")
    _require(scale, torch.float32, "scale")
    _require(shift, torch.float32, "shift")
    if points.dim() != 3 or points.size(2) != 3 or fps_idx.dim() != 2 or fps_idx.size(0) != points.size(0) or subsets.dim() != 2:
        raise RuntimeError("points must be (B,N0,3), fps_idx (B,point_all), subsets (V,npoints)")
    B, N0, _ = points.shape
    P = fps_idx.size(1)
    V, npoints = subsets.shape
    if tuple(scale.shape) != (V, B, 3) or tuple(shift.shape) != (V, B, 3):
        raise RuntimeError("scale and shift must be (V,B,3) = (%d,%d,3)" % (V, B))
    if out is None:
        out = torch.empty(V * B, npoints, 3, dtype=torch.float32, device=points.device)
    _require(out, torch.float32, "out")
    if tuple(out.shape) != (V * B, npoints, 3):
        raise RuntimeError("out must be (V*B,npoints,3)")
    _launch("gm3d_vote_sample", {"B": B, "N0": N0, "point_all": P, "npoints": npoints, "V": V}, lib.gm3d_vote_sample, _ptr(points),
            _ptr(fps_idx), _ptr(subsets), _ptr(scale), _ptr(shift), B, N0, P, npoints, V, _ptr(out), _stream())
    return out


def cls_tail_vote(x, head, labels, V, correct, votes=None):
    """Eval-mode classification head of PointTransformer (cls_head_finetune: Linear, BN, ReLU, Dropout, Linear, BN, ReLU, Dropout,
    Linear) on the stack output x (V*B,T,384) f32/bf16 of all V votes, then the vote mean and its argmax, in one launch.
    head: the nn.Sequential (its parameters and running statistics are read by the kernel on every call).  labels (B,) int64;
    correct: int64 device counter, incremented by the number of correct predictions.  votes: optional (V,B,cls_dim) f32 output.
    -> (mean logits (B,cls_dim) f32, pred (B,) int64)."""
    _require(x, None, "x")
    if x.dtype not in _DT:
        raise RuntimeError("x must be float32 or bfloat16")
    _require(labels, torch.int64, "labels")
    _require(correct, torch.int64, "correct")
    l1, bn1, l2, bn2, l3 = head[0], head[1], head[4], head[5], head[8]
    if bn1.eps != bn2.eps:
        raise RuntimeError("both BatchNorm layers of the head must share eps")
    ps = [l1.weight, l1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
          l2.weight, l2.bias, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var, l3.weight, l3.bias]
    for i, p in enumerate(ps):
        _require(p, torch.float32, "head tensor %d" % i)
    cls_dim = l3.weight.size(0)
    want = [(256, 768)] + [(256,)] * 5 + [(256, 256)] + [(256,)] * 5 + [(cls_dim, 256), (cls_dim,)]
    if [tuple(p.shape) for p in ps] != want:
        raise RuntimeError("head must be Linear(768,256), BN(256), ReLU, Dropout, Linear(256,256), BN(256), ReLU, Dropout, "
                           "Linear(256,cls_dim)")
    if x.dim() != 3 or x.size(0) % V:
        raise RuntimeError("x must be (V*B,T,C)")
    R, T, C = x.shape
    B = R // V
    if labels.numel() != B:
        raise RuntimeError("labels must hold B = %d entries" % B)
    mean = torch.empty(B, cls_dim, dtype=torch.float32, device=x.device)
    pred = torch.empty(B, dtype=torch.int64, device=x.device)
    if votes is not None:
        _require(votes, torch.float32, "votes")
        if tuple(votes.shape) != (V, B, cls_dim):
            raise RuntimeError("votes must be (V,B,cls_dim)")
    _launch("gm3d_cls_tail_vote", {"V": V, "B": B, "T": T, "cls_dim": cls_dim}, lib.gm3d_cls_tail_vote, _ptr(x), int(V), B, T, C,
            *[_ptr(p) for p in ps], cls_dim, float(bn1.eps), _ptr(labels), _ptr(mean), _ptr(pred), _ptr(correct), _ptr(votes),
            _DT[x.dtype], _stream())
    return mean, pred


def _tail_head(head):
    """cls_head_finetune (Linear, BN, ReLU, Dropout, Linear, BN, ReLU, Dropout, Linear) -> (l1, bn1, l2, bn2, l3), checked for the
    kernels' shapes (Linear(F,256), BatchNorm1d(256) x 2 sharing eps and momentum, Linear(256,256), Linear(256,cls_dim))."""
    l1, bn1, l2, bn2, l3 = head[0], head[1], head[4], head[5], head[8]
    ps = [l1.weight, l1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var, l2.weight, l2.bias, bn2.weight, bn2.bias,
          bn2.running_mean, bn2.running_var, l3.weight, l3.bias]
    for i, p in enumerate(ps):
        _require(p, torch.float32, "head tensor %d" % i)
    F, cls_dim = l1.weight.size(1), l3.weight.size(0)
    want = [(256, F)] + [(256,)] * 5 + [(256, 256)] + [(256,)] * 5 + [(cls_dim, 256), (cls_dim,)]
    if [tuple(p.shape) for p in ps] != want:
        raise RuntimeError("head must be Linear(F,256), BN(256), ReLU, Dropout, Linear(256,256), BN(256), ReLU, Dropout, Linear(256,cls_dim)")
    if bn1.eps != bn2.eps or bn1.momentum != bn2.momentum or bn1.momentum is None:
        raise RuntimeError("both BatchNorm layers of the head must share eps and a (non-cumulative) momentum")
    return l1, bn1, l2, bn2, l3


class _ClsTail(torch.autograd.Function):
    """gm3d_cls_tail_fwd / _bwd.  -> logits, or (logits, loss) when labels are given."""

    @staticmethod
    def forward(ctx, x, W1, b1, g1, be1, W2, b2, g2, be2, W3, b3, meta):
        bn1, bn2, mode, training, drop, labels = (meta[k] for k in ("bn1", "bn2", "mode", "training", "drop", "labels"))
        B, T, C = x.shape
        F, cls_dim = W1.size(1), W3.size(0)
        dev = x.device
        feat = torch.empty(B, F, dtype=torch.float32, device=dev)
        argmax = torch.empty(B, C, dtype=torch.int32, device=dev)
        h = torch.empty(2, B, 256, dtype=torch.float32, device=dev)
        stats = torch.empty(4, 256, dtype=torch.float32, device=dev)
        logits = torch.empty(B, cls_dim, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev) if labels is not None else None
        _launch("gm3d_cls_tail_fwd", {"B": B, "T": T, "mode": mode, "cls_dim": cls_dim, "training": training}, lib.gm3d_cls_tail_fwd,
                _ptr(x), B, T, C, mode, *[_ptr(p) for p in (W1, b1, g1, be1, W2, b2, g2, be2, W3, b3)], cls_dim,
                _ptr(bn1.running_mean), _ptr(bn1.running_var), _ptr(bn1.num_batches_tracked), _ptr(bn2.running_mean),
                _ptr(bn2.running_var), _ptr(bn2.num_batches_tracked), float(bn1.eps), float(bn1.momentum), int(training), _ptr(drop),
                _ptr(labels), _ptr(feat), _ptr(argmax), _ptr(h), _ptr(stats), _ptr(logits), _ptr(loss), _DT[x.dtype], _stream())
        ctx.save_for_backward(W1, g1, be1, W2, g2, be2, W3, feat, argmax, h, stats, logits, drop, labels)
        ctx.meta = (B, T, C, mode, training, x.dtype)
        if loss is None:
            return logits
        return logits, loss

    @staticmethod
    def backward(ctx, dlogits, dloss=None):
        W1, g1, be1, W2, g2, be2, W3, feat, argmax, h, stats, logits, drop, labels = ctx.saved_tensors
        B, T, C, mode, training, dt = ctx.meta
        dev = feat.device
        dlogits = dlogits.contiguous().float() if dlogits is not None else None
        dloss = dloss.contiguous().float() if dloss is not None else None
        ws = torch.empty(5, B, 256, dtype=torch.float32, device=dev)
        dx = torch.empty(B, T, C, dtype=dt, device=dev)
        grads = [torch.empty_like(p) for p in (W1, g1, g1, g1, W2, g2, g2, g2, W3)] + [torch.empty(W3.size(0), dtype=torch.float32, device=dev)]
        dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3 = grads
        _launch("gm3d_cls_tail_bwd", {"B": B, "T": T, "mode": mode, "cls_dim": W3.size(0)}, lib.gm3d_cls_tail_bwd, B, T, C, mode,
                *[_ptr(p) for p in (W1, g1, be1, W2, g2, be2, W3)], W3.size(0), int(training), _ptr(drop), _ptr(labels), _ptr(feat),
                _ptr(argmax), _ptr(h), _ptr(stats), _ptr(logits), _ptr(dlogits), _ptr(dloss), _ptr(ws), _ptr(dx),
                *[_ptr(g) for g in grads], _DT[dt], _stream())
        return dx, dW1, db1, dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3, None


def cls_tail(x, head, mode, training, drop=None, labels=None):
    """The Point-M2AE classifiers' tail on our kernels (gm3d_cls_tail_fwd / _bwd: two launches each way): pool the tokens x (B,T,384)
    f32/bf16 -- mode 0: mean + max (F = 384), mode 1: [mean ; max] (F = 768) -- then the head (nn.Sequential cls_head_finetune:
    Linear(F,256), BN, ReLU, Dropout, Linear(256,256), BN, ReLU, Dropout, Linear(256,cls_dim)).  training: batch statistics, the
    running statistics and num_batches_tracked updated in place, drop (2,B,256) f32 dropout factors (or None: no dropout); else the
    running statistics and no dropout.  -> logits (B,cls_dim) f32; with labels (B,) int64 also the mean cross-entropy (a 0-d f32)."""
    _require(x, None, "x")
    if x.dtype not in _DT:
        raise RuntimeError("x must be float32 or bfloat16")
    l1, bn1, l2, bn2, l3 = _tail_head(head)
    if x.dim() != 3 or x.size(2) != 384 or l1.weight.size(1) != (768 if mode else 384):
        raise RuntimeError("x must be (B,T,384) and the head's input width %d for pool mode %d" % (768 if mode else 384, mode))
    B = x.size(0)
    if drop is not None:
        _require(drop, torch.float32, "drop")
        if tuple(drop.shape) != (2, B, 256):
            raise RuntimeError("drop must be (2,B,256)")
    if labels is not None:
        _require(labels, torch.int64, "labels")
        if labels.numel() != B:
            raise RuntimeError("labels must hold B = %d entries" % B)
    meta = {"bn1": bn1, "bn2": bn2, "mode": int(mode), "training": bool(training), "drop": drop if training else None,
            "labels": labels}
    return _ClsTail.apply(x, l1.weight, l1.bias, bn1.weight, bn1.bias, l2.weight, l2.bias, bn2.weight, bn2.bias, l3.weight, l3.bias,
                          meta)


def cls_tail_vote_pool(x, head, mode, labels, V, correct, votes=None, feat=None):
    """cls_tail_vote for the Point-M2AE classifiers (gm3d_cls_tail_vote_pool, one launch): the tokens x (V*B,T,384) f32/bf16 of all V
    votes pooled like cls_tail -- mode 0: mean + max (F = 384), mode 1: [mean ; max] (F = 768), bit for bit -- then the eval-mode
    head (cls_head_finetune with Linear(F,256); parameters and running statistics read on every call), the vote mean and its argmax.
    labels (B,) int64; correct: int64 device counter (+= correct predictions).  votes: optional (V,B,cls_dim) f32 output; feat:
    optional (V*B,F) f32 output of the pooled features.  -> (mean logits (B,cls_dim) f32, pred (B,) int64)."""
    _require(x, None, "x")
    if x.dtype not in _DT:
        raise RuntimeError("x must be float32 or bfloat16")
    _require(labels, torch.int64, "labels")
    _require(correct, torch.int64, "correct")
    if mode not in (0, 1):
        raise RuntimeError("pool mode must be 0 (mean + max) or 1 ([mean ; max])")
    l1, bn1, l2, bn2, l3 = _tail_head(head)
    F = 768 if mode else 384
    if l1.weight.size(1) != F:
        raise RuntimeError("pool mode %d needs a head of input width %d, not %d" % (mode, F, l1.weight.size(1)))
    if x.dim() != 3 or x.size(2) != 384 or x.size(0) % V:
        raise RuntimeError("x must be (V*B,T,384)")
    R, T, C = x.shape
    B = R // V
    cls_dim = l3.weight.size(0)
    if labels.numel() != B:
        raise RuntimeError("labels must hold B = %d entries" % B)
    if votes is not None:
        _require(votes, torch.float32, "votes")
        if tuple(votes.shape) != (V, B, cls_dim):
            raise RuntimeError("votes must be (V,B,cls_dim)")
    if feat is not None:
        _require(feat, torch.float32, "feat")
        if tuple(feat.shape) != (R, F):
            raise RuntimeError("feat must be (V*B,F) = (%d,%d)" % (R, F))
    mean = torch.empty(B, cls_dim, dtype=torch.float32, device=x.device)
    pred = torch.empty(B, dtype=torch.int64, device=x.device)
    _launch("gm3d_cls_tail_vote_pool", {"V": V, "B": B, "T": T, "mode": mode, "cls_dim": cls_dim}, lib.gm3d_cls_tail_vote_pool,
            _ptr(x), int(V), B, T, C, int(mode), *[_ptr(p) for p in (l1.weight, l1.bias, bn1.weight, bn1.bias, bn1.running_mean,
                                                                     bn1.running_var, l2.weight, l2.bias, bn2.weight, bn2.bias,
                                                                     bn2.running_mean, bn2.running_var, l3.weight, l3.bias)],
            cls_dim, float(bn1.eps), _ptr(labels), _ptr(mean), _ptr(pred), _ptr(correct), _ptr(votes), _ptr(feat), _DT[x.dtype],
            _stream())
    return mean, pred


# ------------------------------------------------------------------ KNN / grouping
def knn(ref, query, k, return_dist=True):
    ref = ref.detach().contiguous()
    query = query.detach().contiguous()
    _require(ref, torch.float32, "ref")
    _require(query, torch.float32, "query")
    if ref.dim() != 3 or query.dim() != 3 or ref.size(2) != 3 or query.size(2) != 3 or ref.size(0) != query.size(0):
        raise RuntimeError("ref must be (B,N,3) and query (B,G,3)")
    B, N, _ = ref.shape
    G = query.size(1)
    idx = torch.empty(B, G, k, dtype=torch.int64, device=ref.device)
    dist = torch.empty(B, G, k, dtype=torch.float32, device=ref.device) if return_dist else None
    _launch("gm3d_knn", {"B": B, "N": N, "G": G, "k": int(k)}, lib.gm3d_knn, _ptr(ref), _ptr(query), B, N, G, int(k), _ptr(dist), _ptr(idx), _stream())
    return dist, idx


class KNN(torch.nn.Module):
    """knn_cuda.KNN(k, transpose_mode=True): (ref (B,N,3), query (B,G,3)) -> (dist, idx int64),
    ascending, computed under no_grad like upstream."""

    def __init__(self, k, transpose_mode=False):
        super().__init__()
        self.k = k
        self._t = transpose_mode

    def forward(self, ref, query):
        with torch.no_grad():
            if not self._t:  # upstream's default layout is (B,dim,N)
                ref, query = ref.transpose(1, 2), query.transpose(1, 2)
            dist, idx = knn(ref, query, self.k)
            if not self._t:
                dist, idx = dist.transpose(1, 2).contiguous(), idx.transpose(1, 2).contiguous()
            return dist, idx


def knn_group(xyz, center, k, return_idx=True, return_org=True):
    """Fused Group.forward tail (models_mae_learn_loss.py:946-957):
    -> (neighborhood (B,G,k,3) centred, neighborhood_org | None, idx (B,G,k) int64 | None)."""
    xyz = xyz.detach()
    center = center.detach()
    _require(xyz, torch.float32, "xyz")
    _require(center, torch.float32, "center")
    B, N, _ = xyz.shape
    G = center.size(1)
    dev = xyz.device
    nb = torch.empty(B, G, k, 3, dtype=torch.float32, device=dev)
    nbo = torch.empty(B, G, k, 3, dtype=torch.float32, device=dev) if return_org else None
    idx = torch.empty(B, G, k, dtype=torch.int64, device=dev) if return_idx else None
    _launch("gm3d_knn_group", {"B": B, "N": N, "G": G, "k": int(k)}, lib.gm3d_knn_group, _ptr(xyz), _ptr(center), B, N, G, int(k), _ptr(idx), _ptr(nb), _ptr(nbo), _stream())
    return nb, nbo, idx


# ------------------------------------------------------------------ Chamfer
class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        a = xyz1.contiguous()
        b = xyz2.contiguous()
        _require(a, torch.float32, "xyz1")
        _require(b, torch.float32, "xyz2")
        if a.dim() != 3 or b.dim() != 3 or a.size(2) != 3 or b.size(2) != 3 or a.size(0) != b.size(0):
            raise RuntimeError("xyz1 must be (P,n,3) and xyz2 (P,m,3)")
        P, n, _ = a.shape
        m = b.size(1)
        dev = a.device
        d1 = torch.empty(P, n, dtype=torch.float32, device=dev)
        d2 = torch.empty(P, m, dtype=torch.float32, device=dev)
        i1 = torch.empty(P, n, dtype=torch.int32, device=dev)
        i2 = torch.empty(P, m, dtype=torch.int32, device=dev)
        _launch("gm3d_chamfer_fwd", {"P": P, "n": n, "m": m}, lib.gm3d_chamfer_fwd, _ptr(a), _ptr(b), P, n, m, _ptr(d1), _ptr(d2), _ptr(i1), _ptr(i2), _stream())
        ctx.save_for_backward(a, b, i1, i2)
        ctx.mark_non_differentiable(i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    def backward(ctx, g1, g2, _gi1, _gi2):
        a, b, i1, i2 = ctx.saved_tensors
        P, n, _ = a.shape
        m = b.size(1)
        g1 = g1.contiguous().float() if g1 is not None else None
        g2 = g2.contiguous().float() if g2 is not None else None
        ga = torch.empty_like(a)
        gb = torch.empty_like(b)
        _launch("gm3d_chamfer_bwd", {"P": P, "n": n, "m": m}, lib.gm3d_chamfer_bwd, _ptr(a), _ptr(b), _ptr(i1), _ptr(i2), _ptr(g1), _ptr(g2), P, n, m,
                                   _ptr(ga), _ptr(gb), _stream())
        return ga, gb


def chamfer(xyz1, xyz2):
    """-> (dist1 (P,n), dist2 (P,m), idx1 int32, idx2 int32); differentiable wrt both clouds."""
    return _Chamfer.apply(xyz1, xyz2)


class ChamferDistanceL2(torch.nn.Module):
    """extensions.chamfer_dist.ChamferDistanceL2.

    reduction='per_point' (default) is the GM3D-local form the hot path needs
    (models_mae_learn_loss.py:407-412 reshapes the result to (N,-1,n)): a (P,n) tensor
    dist1 + dist2, n == m.  The exact combination is not recoverable from the reference
    tree -- parity unpinned.  reduction='mean' is the upstream scalar
    mean(dist1) + mean(dist2) used by models/Point_MAE.py:426.
    """

    def __init__(self, ignore_zeros=False, reduction="per_point"):
        super().__init__()
        self.ignore_zeros = ignore_zeros
        self.reduction = reduction

    def forward(self, xyz1, xyz2):
        if self.ignore_zeros and xyz1.size(0) == 1:  # upstream's batch-1 zero filter
            xyz1 = xyz1[torch.sum(xyz1, dim=2).ne(0)].unsqueeze(0)
            xyz2 = xyz2[torch.sum(xyz2, dim=2).ne(0)].unsqueeze(0)
        d1, d2, _, _ = chamfer(xyz1, xyz2)
        if self.reduction == "per_point":
            if d1.shape != d2.shape:
                raise RuntimeError("per_point Chamfer needs n == m")
            return d1 + d2
        return torch.mean(d1) + torch.mean(d2)


class ChamferDistanceL1(torch.nn.Module):
    def __init__(self, ignore_zeros=False):
        super().__init__()
        self.ignore_zeros = ignore_zeros

    def forward(self, xyz1, xyz2):
        if self.ignore_zeros and xyz1.size(0) == 1:
            xyz1 = xyz1[torch.sum(xyz1, dim=2).ne(0)].unsqueeze(0)
            xyz2 = xyz2[torch.sum(xyz2, dim=2).ne(0)].unsqueeze(0)
        d1, d2, _, _ = chamfer(xyz1, xyz2)
        return (torch.mean(torch.sqrt(d1)) + torch.mean(torch.sqrt(d2))) / 2


# ------------------------------------------------------------------ attention
_DT = {torch.float32: _capi.GM3D_F32, torch.bfloat16: _capi.GM3D_BF16}


def attention(qkv, num_heads, scale):
    """qkv (B,T,3*H*64) = output of the qkv Linear (timm layout (B,T,3,H,64)) -> (B,T,H*64).  T <= 128: one workgroup per (cloud,
    head) with the whole head in LDS; 128 < T <= 512 (cfgs/config_3.yaml: 256 groups): the flash-style kernel of the hierarchical
    encoder without a mask; 513 <= T <= 2048 (the 8k recipe: 512 groups + the class token): its streaming form."""
    return _attention.AttentionFn.apply(qkv, None, num_heads, scale, True, True)


def pack_mask(mask):
    """(B,T,T) bool, True = pair not allowed -> (B,T,ceil(T/32)) int32 bitset for attention_masked (bit j&31 of word j>>5)."""
    B, T, _ = mask.shape
    W = (T + 31) // 32
    m = torch.ones(B, T, W * 32, dtype=torch.int64, device=mask.device)      # keys past T: blocked (the kernels force them anyway)
    m[:, :, :T] = mask.to(torch.int64)
    weights = (torch.ones(32, dtype=torch.int64, device=mask.device) << torch.arange(32, device=mask.device))
    words = (m.view(B, T, W, 32) * weights).sum(-1)                     # 0 .. 2^32-1
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


def radius_mask_bits(center, vis, radius, masked=None):
    """center (B,G,3) f32, vis (B,G) bool | None -> (B,G,ceil(G/32)) int32 bitset: pair (i,j) blocked iff i or j invisible or their
    centres are >= radius apart (== pack_mask(~(vis_i & vis_j) | dist2 >= radius^2), in one launch and without the (B,G,G) tensors).
    masked (B,G) bool (True = NOT visible) may be given instead of vis (no bitwise_not, no converting copy)."""
    center = center.detach().contiguous()
    _require(center, torch.float32, "center")
    B, G, _ = center.shape
    inv = 0
    if masked is not None and vis is None:
        v = masked.contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v.to(torch.uint8)
        inv = 1
    elif vis is not None:
        v = vis.contiguous()
        v = v.view(torch.uint8) if v.dtype == torch.bool else v.to(torch.uint8)
    else:
        v = None
    bits = torch.empty(B, G, (G + 31) // 32, dtype=torch.int32, device=center.device)
    _launch("gm3d_radius_mask_bits", {"B": B, "G": G}, lib.gm3d_radius_mask_bits_m, _ptr(center), _ptr(v), inv, float(radius), B, G,
            _ptr(bits), _stream())
    return bits


def attention_masked(qkv, bits, num_heads, scale):
    """qkv (B,T,3*H*hd), hd in {16,32,64}, T <= 2048; bits = pack_mask(mask) of a SYMMETRIC (B,T,T) bool mask (True = not allowed)
    or None -> (B,T,H*hd).  A query with no allowed key yields zeros.  (The hierarchical Point-M2AE encoder's attention.)
    T <= 512: the head sits in LDS (csrc/attention_masked.hip); 513 <= T <= 2048: it streams through (csrc/attention_long.hip)."""
    return _attention.AttentionFn.apply(qkv, bits, num_heads, scale, False, False)


# ------------------------------------------------------------------ reconstructed clouds (models/Point_MAE.py:428-439)
@torch.no_grad()
def reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=False):
    """The `vis` branch of the reference's Point_MAE.forward in one launch (gm3d_reconstruct_assemble): pred (B,M,3k) f32/bf16 -- a
    batch-strided view such as pix_pred[:, -M:] is taken as it is --, neighborhood (B,G,k,3) f32 centre-relative, center (B,G,3) f32,
    vis_ids (B,V) / mask_ids (B,M) int64 (row-strided views are taken as they are), V + M = G
    -> (dense (B*G*k,3) f32, full_center (B*G,3) f32), detached (there is no backward).
    flat=False: per cloud, [visible patches in vis_ids order | rebuilt patches in mask_ids order], full_center in the same order.
    flat=True: the reference's layout -- all clouds' visible patches, then all rebuilt ones; full_center all MASKED centres, then all
    visible ones."""
    neighborhood, center = neighborhood.detach(), center.detach()
    _require(neighborhood, torch.float32, "neighborhood")
    _require(center, torch.float32, "center")
    _require(vis_ids, torch.int64, "vis_ids", contiguous=False)
    _require(mask_ids, torch.int64, "mask_ids", contiguous=False)
    if neighborhood.dim() != 4 or neighborhood.size(3) != 3 or tuple(center.shape) != tuple(neighborhood.shape[:2]) + (3,):
        raise RuntimeError("neighborhood must be (B,G,k,3) and center (B,G,3)")
    B, G, k, _ = neighborhood.shape
    if vis_ids.dim() != 2 or mask_ids.dim() != 2 or vis_ids.size(0) != B or mask_ids.size(0) != B:
        raise RuntimeError("vis_ids must be (B,V) and mask_ids (B,M)")
    V, M = vis_ids.size(1), mask_ids.size(1)
    if V + M != G:
        raise RuntimeError("V + M = %d + %d must equal G = %d" % (V, M, G))
    if (V > 1 and vis_ids.stride(1) != 1) or (M > 1 and mask_ids.stride(1) != 1):
        raise RuntimeError("the id rows must be dense (stride 1 along dim 1)")
    dt = _capi.GM3D_F32
    if M > 0:
        pred = pred.detach()
        _require(pred, None, "pred", contiguous=False)
        if pred.dtype not in _DT:
            raise RuntimeError("pred must be float32 or bfloat16")
        if tuple(pred.shape) != (B, M, 3 * k) or pred.stride(2) != 1 or pred.stride(1) != 3 * k:
            raise RuntimeError("pred must be (B,M,3k) = (%d,%d,%d) with dense rows" % (B, M, 3 * k))
        dt = _DT[pred.dtype]
    dense = torch.empty(B * G * k, 3, dtype=torch.float32, device=neighborhood.device)
    full_center = torch.empty(B * G, 3, dtype=torch.float32, device=neighborhood.device)
    if B == 0:
        return dense, full_center

    def bstride(t, need):          # a batch of one may carry any stride along dim 0
        return t.stride(0) if B > 1 else max(t.stride(0), need)
    _launch("gm3d_reconstruct_assemble", {"B": B, "G": G, "k": k, "M": M, "flat": bool(flat)}, lib.gm3d_reconstruct_assemble,
            _ptr(pred) if M > 0 else None, bstride(pred, M * 3 * k) if M > 0 else 0, _ptr(neighborhood), _ptr(center),
            _ptr(vis_ids) if V > 0 else None, bstride(vis_ids, V) if V > 0 else 0, _ptr(mask_ids) if M > 0 else None,
            bstride(mask_ids, M) if M > 0 else 0, B, G, k, V, M, 1 if flat else 0, _ptr(dense), _ptr(full_center), dt, _stream())
    return dense, full_center


@torch.no_grad()
def reconstruct_partition(pred, neighborhood, center, masked):
    """The ragged form for the hierarchical model, one launch (gm3d_reconstruct_partition): a stable per-cloud partition of the tokens
    by `masked` (B,G) bool or uint8 (non-zero = masked) with the patches moved back to their centres in that order.  neighborhood
    (B,G,k,3) f32 centre-relative, center (B,G,3) f32; pred (B,G,3k) f32/bf16 contiguous with a row for EVERY token (rows of visible
    tokens are never read), or None: a masked token's rows are then its true patch.
    -> (dense (B,G*k,3) f32: per cloud [visible patches | masked patches], each in ascending token index; full_center (B,G,3) f32 and
    order (B,G) int32 (the token at each slot) in the same order; n_visible (B,) int32), detached (there is no backward)."""
    neighborhood, center = neighborhood.detach(), center.detach()
    _require(neighborhood, torch.float32, "neighborhood")
    _require(center, torch.float32, "center")
    _require(masked, None, "masked")
    if neighborhood.dim() != 4 or neighborhood.size(3) != 3 or tuple(center.shape) != tuple(neighborhood.shape[:2]) + (3,):
        raise RuntimeError("neighborhood must be (B,G,k,3) and center (B,G,3)")
    B, G, k, _ = neighborhood.shape
    if masked.dtype not in (torch.bool, torch.uint8) or tuple(masked.shape) != (B, G):
        raise RuntimeError("masked must be (B,G) = (%d,%d) bool or uint8" % (B, G))
    dt = _capi.GM3D_F32
    if pred is not None:
        pred = pred.detach()
        _require(pred, None, "pred")
        if pred.dtype not in _DT:
            raise RuntimeError("pred must be float32 or bfloat16")
        if tuple(pred.shape) != (B, G, 3 * k):
            raise RuntimeError("pred must be (B,G,3k) = (%d,%d,%d): a row for every token" % (B, G, 3 * k))
        dt = _DT[pred.dtype]
    dev = neighborhood.device
    dense = torch.empty(B, G * k, 3, dtype=torch.float32, device=dev)
    full_center = torch.empty(B, G, 3, dtype=torch.float32, device=dev)
    order = torch.empty(B, G, dtype=torch.int32, device=dev)
    n_visible = torch.empty(B, dtype=torch.int32, device=dev)
    if B == 0:
        return dense, full_center, order, n_visible
    _launch("gm3d_reconstruct_partition", {"B": B, "G": G, "k": k, "pred": pred is not None}, lib.gm3d_reconstruct_partition,
            _ptr(pred), _ptr(neighborhood), _ptr(center), _ptr(masked), B, G, k, dt, _ptr(dense), _ptr(full_center), _ptr(order),
            _ptr(n_visible), _stream())
    return dense, full_center, order, n_visible


# which kernel runs attention, and the autograd node of the two ops above; at the end: it imports this module's helpers
from . import attention as _attention  # noqa: E402

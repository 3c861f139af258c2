"""Soft-target losses and point mixup for the classification fine-tune ("Soft targets").

  soft_cross_entropy          the autograd node over gm3d_soft_ce_fwd / _bwd (gm3d_amd/csrc/soft_ce.hip): one launch each way
  SoftTargetCrossEntropy      timm's: sum(-t * log_softmax(x), -1).mean() for dense targets
  LabelSmoothingCrossEntropy  timm's convention (Point-MAE_SA3D/main_finetune.py:369-375): on 1 - s + s / C, off s / C
  SmoothLoss                  Point-M2AE's convention (DGCNN cal_loss; `smooth: 0.3` of finetune_modelnet_PointM2AE.yaml): on 1 - eps,
                              off eps / (C - 1)
  PointMixup, MixedTargets    Point-MAE_SA3D/engine_finetune.py:43-76 (mixup_point_cloud) as one launch (gm3d_mixup_points)

A target row is handed to the kernels in compact form, t_ic = u + wa [c = ya_i] + wb [c = yb_i] with coef = (wa, wb, u) =
((on - off) lam, (on - off) (1 - lam), off): the host computes the three numbers in double and delivers them through a
streams.PinnedFeed into a device tensor the loss owns, so nothing of a draw is baked into a captured graph -- before a replay the
step calls stage(lam) (engine_finetune.GraphedFinetuneStep does).  CPU tensors take the same formulas in plain torch (tests; there is
no CPU path for the kernels themselves)."""
import numpy as np
import torch
import torch.nn as nn

from . import streams


def _is_capturing(t):
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def _device(device):
    """torch.device with the index filled in ("cuda" -> the current device), so that it compares equal to a tensor's"""
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


# --------------------------------------------------------------------------- the node
def _check(logits, ya, yb, coef, dense):
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("logits must be (B,C) float32 or bfloat16")
    B, C = logits.shape
    if (dense is None) == (ya is None and yb is None and coef is None):
        raise ValueError("give the targets in exactly one form: (ya, [yb,] coef) or dense")
    if dense is not None:
        if dense.dtype != torch.float32 or tuple(dense.shape) != (B, C) or dense.device != logits.device:
            raise RuntimeError("dense must be (B,C) float32 on the logits' device")
        return
    if ya is None or coef is None:
        raise ValueError("the compact form needs ya and coef")
    for name, y in (("ya", ya), ("yb", yb)):
        if y is not None and (y.dtype != torch.int64 or y.numel() != B or y.device != logits.device):
            raise RuntimeError("%s must hold B = %d int64 labels on the logits' device" % (name, B))
    if coef.dtype != torch.float32 or coef.numel() != 3 or coef.device != logits.device:
        raise RuntimeError("coef must be (3,) float32 = (wa, wb, u) on the logits' device")


def soft_ce_forward(logits, ya=None, yb=None, coef=None, dense=None):
    """gm3d_soft_ce_fwd on contiguous GPU tensors -> (loss 0-d, row_loss (B,), lse (B,)), all f32.  No autograd."""
    from . import ops
    from ._capi import lib
    _check(logits, ya, yb, coef, dense)
    if not all(t is None or t.is_contiguous() for t in (logits, ya, yb, coef, dense)):
        raise RuntimeError("soft_ce_forward takes contiguous tensors")
    B, C = logits.shape
    row_loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    lse = torch.empty(B, dtype=torch.float32, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    ops._launch("gm3d_soft_ce_fwd", {"B": B, "C": C}, lib.gm3d_soft_ce_fwd, ops._ptr(logits), B, C, ops._ptr(ya), ops._ptr(yb),
                ops._ptr(coef), ops._ptr(dense), ops._ptr(row_loss), ops._ptr(lse), ops._ptr(loss), ops._DT[logits.dtype], ops._stream())
    return loss, row_loss, lse


def soft_ce_backward(logits, lse, dloss, ya=None, yb=None, coef=None, dense=None):
    """gm3d_soft_ce_bwd on the forward's tensors -> dlogits in the logits' dtype.  lse: the forward's; dloss: 0-d / (1,) f32 on the
    device."""
    from . import ops
    from ._capi import lib
    B, C = logits.shape
    dlogits = torch.empty_like(logits)
    ops._launch("gm3d_soft_ce_bwd", {"B": B, "C": C}, lib.gm3d_soft_ce_bwd, ops._ptr(logits), B, C, ops._ptr(ya), ops._ptr(yb),
                ops._ptr(coef), ops._ptr(dense), ops._ptr(lse), ops._ptr(dloss), ops._ptr(dlogits), ops._DT[logits.dtype], ops._stream())
    return dlogits


class _SoftCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, ya, yb, coef, dense):
        logits, dense = logits.contiguous(), None if dense is None else dense.contiguous()
        ya, yb = (None if y is None else y.reshape(-1).contiguous() for y in (ya, yb))
        loss, _, lse = soft_ce_forward(logits, ya, yb, coef, dense)
        ctx.save_for_backward(logits, ya, yb, coef, dense, lse)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, ya, yb, coef, dense, lse = ctx.saved_tensors
        return soft_ce_backward(logits, lse, dloss.contiguous().float(), ya, yb, coef, dense), None, None, None, None


def _soft_ce_cpu(logits, ya, yb, coef, dense):
    """The kernels' formulas in plain torch (f32): row = sum_c t_c (lse - z_c), a label outside [0, C) -> NaN."""
    z = logits.float()
    C = z.size(1)
    m = z.max(dim=1, keepdim=True)[0]
    lse = m + torch.log(torch.exp(z - m).sum(dim=1, keepdim=True))
    d = lse - z
    if dense is not None:
        return (dense * d).sum(dim=1).mean()
    wa, wb, u = coef[0], coef[1], coef[2]

    def pick(y):
        ok = (y >= 0) & (y < C)
        v = d.gather(1, y.clamp(0, C - 1).view(-1, 1)).squeeze(1)
        return torch.where(ok, v, torch.full_like(v, float("nan")))
    row = wa * pick(ya.reshape(-1))
    if yb is not None:
        row = row + wb * pick(yb.reshape(-1))
    return (row + u * d.sum(dim=1)).mean()


def soft_cross_entropy(logits, ya=None, yb=None, coef=None, dense=None):
    """Mean over the B rows of sum_c t_ic (lse_i - z_ic) -> a 0-d f32 loss, differentiable in the logits.
    logits (B,C) f32 / bf16.  The targets in exactly one form: compact -- ya (B,) int64, yb (B,) int64 or None, coef (3,) f32 on the
    logits' device = (wa, wb, u), t_ic = u + wa [c = ya_i] + wb [c = yb_i] -- or dense (B,C) f32.  The rows need not sum to 1.
    GPU: gm3d_soft_ce_fwd / _bwd, one launch each, B <= 4096 and C <= 1024; CPU: the same formulas in plain torch."""
    _check(logits, ya, yb, coef, dense)
    if not logits.is_cuda:
        return _soft_ce_cpu(logits, ya, yb, coef, dense)
    return _SoftCE.apply(logits, ya, yb, coef, dense)


# --------------------------------------------------------------------------- mixed targets
class MixedTargets:
    """The targets of a mixed batch: lam * onehot(ya) + (1 - lam) * onehot(yb).  ya, yb (B,) int64; coef2 (2,) f32 on their device =
    (f32(lam), f32(1 - lam)), what the mixing launch read; lam: the host's draw (a Python float) the losses form their coefficients
    from -- inside a captured step it is the draw of the capture, and the step re-stages the loss before every replay."""

    def __init__(self, ya, yb, coef2, lam):
        self.ya, self.yb, self.coef2, self.lam = ya, yb, coef2, float(lam)

    def long(self):
        return self

    def dense(self, num_classes):
        """(B,num_classes) f32, the reference's mixed_labels_onehot (its 15 classes replaced by the caller's count)."""
        one = torch.nn.functional.one_hot
        return self.coef2[0] * one(self.ya, num_classes).float() + self.coef2[1] * one(self.yb, num_classes).float()


# --------------------------------------------------------------------------- the losses
class _CompactTargetLoss(nn.Module):
    """int64 labels or MixedTargets -> the compact form.  Subclasses give on_off(C)."""

    def __init__(self):
        super().__init__()
        self._coef, self._feed, self._staged, self._classes = None, None, None, None

    def on_off(self, C):
        raise NotImplementedError

    def coefficients(self, C, lam=1.0):
        """(wa, wb, u) = ((on - off) lam, (on - off) (1 - lam), off), formed in double, rounded once to f32."""
        on, off = self.on_off(int(C))
        lam = float(lam)
        return np.array([(on - off) * lam, (on - off) * (1.0 - lam), off], dtype=np.float64).astype(np.float32)

    def stage(self, lam=1.0, num_classes=None, device=None):
        """The coefficients for `lam` -> this loss's device tensor, on the current stream.  num_classes / device default to the last
        forward's.  A captured step calls this before each replay; forward() calls it itself outside a capture."""
        if self._coef is None and (num_classes is None or device is None):
            raise RuntimeError("stage() before the first forward needs num_classes and device")
        C = self._classes if num_classes is None else int(num_classes)
        device = self._coef.device if device is None else _device(device)
        key = (C, float(lam), device)
        if key == self._staged:
            return self._coef
        arr = self.coefficients(C, lam)
        if device.type != "cuda":
            self._coef, self._feed = torch.from_numpy(arr.copy()), None
        else:
            if self._coef is None or self._coef.device != device:
                self._coef = torch.zeros(3, dtype=torch.float32, device=device)
                self._feed = streams.PinnedFeed(self._coef)
            self._feed.push([arr])
        self._staged, self._classes = key, C
        return self._coef

    def forward(self, logits, target):
        C = logits.size(-1)
        mixed = isinstance(target, MixedTargets)
        ya, yb = (target.ya, target.yb) if mixed else (target, None)
        if _is_capturing(logits):       # the coefficients are a static input of the capture: staged before, re-staged per replay
            if self._coef is None or self._coef.device != logits.device or self._classes != C:
                raise RuntimeError("%s: run one eager step (or stage()) before capturing" % type(self).__name__)
        else:
            self.stage(target.lam if mixed else 1.0, C, logits.device)
        return soft_cross_entropy(logits, ya=ya, yb=yb, coef=self._coef)


class SoftTargetCrossEntropy(_CompactTargetLoss):
    """timm.loss.SoftTargetCrossEntropy: sum(-target * log_softmax(x, -1), -1).mean() for dense (B,C) targets (any row sums).
    MixedTargets and int64 labels are taken as the one-hot rows they stand for."""

    def on_off(self, C):
        return 1.0, 0.0

    def forward(self, logits, target):
        if torch.is_tensor(target) and target.is_floating_point():
            return soft_cross_entropy(logits, dense=target.float())
        return super().forward(logits, target)


class LabelSmoothingCrossEntropy(_CompactTargetLoss):
    """timm.loss.LabelSmoothingCrossEntropy(smoothing): (1 - s) * nll + s * mean_c(-log p), i.e. on-value 1 - s + s / C, off-value s / C."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError("smoothing must be in [0, 1)")
        self.smoothing = float(smoothing)

    def on_off(self, C):
        return 1.0 - self.smoothing + self.smoothing / C, self.smoothing / C


class SmoothLoss(_CompactTargetLoss):
    """Point-M2AE's smoothed cross-entropy (DGCNN cal_loss): on-value 1 - eps, off-value eps / (C - 1)."""

    def __init__(self, eps=0.3):
        super().__init__()
        if not 0.0 <= eps < 1.0:
            raise ValueError("eps must be in [0, 1)")
        self.eps = float(eps)

    def on_off(self, C):
        if C < 2:
            raise ValueError("SmoothLoss spreads eps over the other C - 1 classes: C = %d has none" % C)
        return 1.0 - self.eps, self.eps / (C - 1)


# --------------------------------------------------------------------------- mixup
class PointMixup:
    """mixup_point_cloud(data, alpha, labels) of Point-MAE_SA3D/engine_finetune.py:43-76.
    draw(B): lam = rng.beta(alpha, alpha), then torch.randperm(B, generator=generator) -- the reference's order of draws -- staged on
    the device as coef2 = (f32(lam), f32(1 - lam)) and perm; mix(points, targets): lam * points + (1 - lam) * points[perm] and
    MixedTargets(targets, targets[perm]) from the staged draw, one launch on the GPU (gm3d_mixup_points), the reference's expression
    on the CPU; __call__ = draw + mix.  The class count comes from the logits the loss sees, not from the reference's fixed 15."""

    def __init__(self, alpha, rng=np.random, generator=None):
        if not alpha > 0:
            raise ValueError("alpha must be positive")
        self.alpha, self.rng, self.generator = float(alpha), rng, generator
        self.lam = None
        self._dev = {}             # (B, device) -> (coef2, perm, feed)

    def draw(self, B, device="cpu", lam=None, perm=None):
        """The host draw (lam / perm inject it: tests, parity) -> (lam, perm), staged for `device` on the current stream."""
        lam = float(self.rng.beta(self.alpha, self.alpha)) if lam is None else float(lam)
        perm = torch.randperm(B, generator=self.generator) if perm is None else torch.as_tensor(perm, dtype=torch.long).cpu()
        if perm.numel() != B or (B > 0 and (int(perm.min()) < 0 or int(perm.max()) >= B)):
            raise ValueError("perm must hold B = %d indices in [0, B)" % B)
        self.lam = lam
        device = _device(device)
        c2 = np.array([lam, 1.0 - lam], dtype=np.float64).astype(np.float32)
        if device.type != "cuda":
            self._dev[(B, device)] = (torch.from_numpy(c2), perm.clone(), None)
            return lam, perm
        slot = self._dev.get((B, device))
        if slot is None:
            coef2 = torch.tensor([1.0, 0.0], dtype=torch.float32, device=device)
            dperm = torch.arange(B, dtype=torch.long, device=device)
            slot = self._dev[(B, device)] = (coef2, dperm, streams.PinnedFeed(coef2, dperm))
        slot[2].push([c2, perm.numpy()])
        return lam, perm

    def mix(self, points, targets):
        """The staged draw applied: points (B,N,3) f32, targets (B,) int -> (mixed points, MixedTargets)."""
        B = points.size(0)
        slot = self._dev.get((B, points.device))
        if slot is None:
            raise RuntimeError("PointMixup.mix: no draw staged for B = %d on %s" % (B, points.device))
        coef2, perm, _ = slot
        ya = targets.reshape(-1).long()
        if not points.is_cuda:
            lam = self.lam
            return lam * points + (1 - lam) * points[perm], MixedTargets(ya, ya[perm], coef2, lam)
        from . import ops
        from ._capi import lib
        if points.dim() != 3 or points.size(2) != 3 or points.dtype != torch.float32:
            raise RuntimeError("points must be (B,N,3) float32")
        points, ya = points.contiguous(), ya.contiguous()
        out = torch.empty_like(points)
        yb = torch.empty_like(ya)
        N = points.size(1)
        ops._launch("gm3d_mixup_points", {"B": B, "N": N}, lib.gm3d_mixup_points, ops._ptr(points), B, N, ops._ptr(perm), ops._ptr(coef2),
                    ops._ptr(ya), ops._ptr(out), ops._ptr(yb), ops._stream())
        return out, MixedTargets(ya, yb, coef2, self.lam)

    def __call__(self, points, targets):
        self.draw(points.size(0), points.device)
        return self.mix(points, targets)

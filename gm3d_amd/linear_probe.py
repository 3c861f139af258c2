"""Linear probe of pretrained features on the MI355X: Point-MAE_SA3D/main_linprob.py:219-263, the third quality signal beside the
linear SVM and the weighted k-NN vote (validate.evaluate_linear).

A frozen encoder's pooled features -> BatchNorm1d(affine=False, eps=1e-6) -> Linear, trained with SGD + momentum on the cross-entropy,
warm-up + half-cosine rate (util/lr_sched.adjust_learning_rate at epoch + it / iterations_per_epoch), the rows of epoch e in the order
of the reference's DistributedSampler (data.epoch_order(n, e, True, seed, 0, 1)), consecutive batches, drop_last=True.  All fp32: the
reference's fp16 autocast is not reproduced.  One launch per training iteration (plus one per evaluated segment) and one per
evaluation; the rates, the orders and the initial weights are made on the host and copied once; nothing is read back before the fit
ends, then one read of the (epochs, 2) hit table.  Bitwise reproducible.  The contracts are in include/gm3d.h; there is no CPU path.

The evaluation runs over ALL test rows: the reference's drop_last=True on its validation loader is an ImageNet-loader quirk and is
not copied.
"""
import math

import torch

from . import _capi
from .data import epoch_order
from .ops import _ptr, _stream

MAX_N, MIN_D, MAX_D, D_MULTIPLE, MAX_CLASSES, MAX_BATCH = 16384, 8, 1024, 8, 64, 1024


def _require_cuda(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU path)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous %s tensor" % (name, dtype))


def _features(t, name):
    _require_cuda(t, torch.float32, name)
    if t.dim() != 2:
        raise ValueError("%s must be (rows, channels), got %s" % (name, tuple(t.shape)))


def learning_rates(epochs, ipe, lr, min_lr, warmup_epochs):
    """util/lr_sched.adjust_learning_rate at e + it / ipe for every iteration, in double on the host -> list of epochs * ipe rates."""
    out = []
    for e in range(epochs):
        for it in range(ipe):
            x = e + it / ipe
            if x < warmup_epochs:
                out.append(lr * x / warmup_epochs)
            else:
                out.append(min_lr + (lr - min_lr) * 0.5 * (1.0 + math.cos(math.pi * (x - warmup_epochs) / (epochs - warmup_epochs))))
    return out


class LinearProbe:
    """main_linprob.py's head and its training loop on cached features.  After fit: weight (C,d), bias (C), running_mean (d),
    running_var (d), losses (epochs * (n // batch_size)) on the device, history [(top-1 %, top-5 %)] per evaluated epoch and
    eval_epochs, their 1-based epochs.  lr None: blr * batch_size / 256."""

    def __init__(self, num_classes, batch_size=512, epochs=90, warmup_epochs=10, blr=0.1, lr=None, min_lr=0.0, momentum=0.9, seed=0,
                 eval_every=1):
        if not 2 <= num_classes <= MAX_CLASSES:
            raise ValueError("num_classes must be in 2..%d" % MAX_CLASSES)
        if not 2 <= batch_size <= MAX_BATCH:
            raise ValueError("batch_size must be in 2..%d" % MAX_BATCH)
        if epochs < 1 or eval_every < 1 or warmup_epochs < 0 or not 0.0 <= momentum < 1.0:
            raise ValueError("epochs >= 1, eval_every >= 1, warmup_epochs >= 0 and 0 <= momentum < 1")
        self.num_classes, self.batch_size, self.epochs, self.warmup_epochs = int(num_classes), int(batch_size), int(epochs), warmup_epochs
        self.lr = blr * batch_size / 256 if lr is None else lr
        self.min_lr, self.momentum, self.seed, self.eval_every = min_lr, momentum, int(seed), int(eval_every)
        self.weight = self.bias = self.running_mean = self.running_var = self.losses = None
        self.history, self.eval_epochs = [], []

    def _labels(self, labels, rows, name):
        labels = labels.view(-1)
        _require_cuda(labels, torch.int64, name)
        if labels.numel() != rows:
            raise ValueError("%s: %d labels for %d rows" % (name, labels.numel(), rows))
        return labels

    def fit(self, train_features, train_labels, test_features=None, test_labels=None, weight=None, orders=None):
        """weight (C,d) f32: the initial weights instead of trunc_normal_(std=0.01) on a generator seeded with `seed`.
        orders: `epochs` lists of row indices instead of the sampler's; the first (n // batch_size) * batch_size of each are used."""
        _features(train_features, "train_features")
        X, (n, d), C, B, E = train_features, train_features.shape, self.num_classes, self.batch_size, self.epochs
        y = self._labels(train_labels, n, "train_labels")
        if not (1 <= n <= MAX_N and MIN_D <= d <= MAX_D and d % D_MULTIPLE == 0):
            raise ValueError("1 <= n <= %d, %d <= d <= %d, d %% %d == 0: got n = %d, d = %d" % (MAX_N, MIN_D, MAX_D, D_MULTIPLE, n, d))
        if B > n:
            raise ValueError("batch_size %d above the %d training rows" % (B, n))
        Q = yq = None
        if test_features is not None:
            _features(test_features, "test_features")
            if test_features.shape[1] != d:
                raise ValueError("train and test features disagree: %d vs %d channels" % (d, test_features.shape[1]))
            Q, yq = test_features, self._labels(test_labels, test_features.shape[0], "test_labels")
        dev, ipe = X.device, n // B
        T = E * ipe
        lo, hi = y.min(), y.max()
        if yq is not None and yq.numel():
            lo, hi = torch.minimum(lo, yq.min()), torch.maximum(hi, yq.max())
        bad = ((lo < 0) | (hi >= C)).view(1).to(torch.int64)       # stays on the device: read with the hit table
        # host side, copied once: orders, rates, initial weights
        if orders is None:
            orders = [epoch_order(n, e, True, self.seed, 0, 1) for e in range(E)]
        if len(orders) != E:
            raise ValueError("%d orders for %d epochs" % (len(orders), E))
        flat = []
        for o in orders:
            o = [int(v) for v in o][:ipe * B]
            if len(o) != ipe * B or (o and not 0 <= min(o) <= max(o) < n):
                raise ValueError("every order holds at least %d row indices in 0..%d" % (ipe * B, n - 1))
            flat += o
        order = torch.tensor(flat, dtype=torch.int32).to(dev)
        rates = torch.tensor(learning_rates(E, ipe, self.lr, self.min_lr, self.warmup_epochs), dtype=torch.float64).float().to(dev)
        if weight is None:
            w0 = torch.empty(C, d, dtype=torch.float32)
            torch.nn.init.trunc_normal_(w0, std=0.01, generator=torch.Generator().manual_seed(self.seed))
        else:
            if tuple(weight.shape) != (C, d):
                raise ValueError("weight must be (%d, %d), got %s" % (C, d, tuple(weight.shape)))
            w0 = weight.detach().float()
        W = w0.to(dev).contiguous().clone()
        mom_w, bias2, mom_b = torch.zeros_like(W), torch.zeros(2, C, device=dev), torch.zeros(C, device=dev)
        rmean, rvar = torch.zeros(d, device=dev), torch.ones(d, device=dev)
        xhat = torch.empty(B, d, dtype=torch.float32, device=dev)
        part = torch.empty(2 * _capi.lib.gm3d_linprobe_slices(d) * C * B, dtype=torch.float32, device=dev)
        losses = torch.empty(T, dtype=torch.float32, device=dev)
        evals = [e for e in range(1, E + 1) if e % self.eval_every == 0 or e == E] if Q is not None else []
        table = torch.zeros(max(len(evals), 1), 2, dtype=torch.int64, device=dev)
        stream, done = _stream(), 0
        for k, e in enumerate(evals or [E]):
            _capi.check(_capi.lib.gm3d_linprobe_train(_ptr(X), _ptr(y), n, d, C, B, _ptr(order), _ptr(rates), done, e * ipe,
                                                      float(self.momentum), _ptr(W), _ptr(mom_w), _ptr(bias2), _ptr(mom_b), _ptr(rmean),
                                                      _ptr(rvar), _ptr(xhat), _ptr(part), _ptr(losses), stream), "gm3d_linprobe_train")
            done = e * ipe
            if evals:
                _capi.check(_capi.lib.gm3d_linprobe_eval(_ptr(Q), _ptr(yq), Q.shape[0], d, C, _ptr(W), _ptr(bias2[done & 1]), _ptr(rmean),
                                                         _ptr(rvar), None, None, _ptr(table[k]), stream), "gm3d_linprobe_eval")
        out = torch.cat([table.view(-1), bad]).tolist()            # the one read
        if out[-1]:
            raise ValueError("labels outside 0..%d" % (C - 1))
        total = max(Q.shape[0], 1) if Q is not None else 1
        self.history = [(out[2 * k] * 100.0 / total, out[2 * k + 1] * 100.0 / total) for k in range(len(evals))]
        self.eval_epochs = evals
        self.weight, self.bias, self.running_mean, self.running_var, self.losses = W, bias2[T & 1].clone(), rmean, rvar, losses
        return self

    def _eval(self, features, labels, want_pred):
        if self.weight is None:
            raise RuntimeError("fit first")
        _features(features, "features")
        m, d = features.shape
        if d != self.weight.shape[1]:
            raise ValueError("features have %d channels, the probe %d" % (d, self.weight.shape[1]))
        pred = torch.empty(m, dtype=torch.int64, device=features.device) if want_pred else None
        correct = None
        if labels is not None:
            labels = self._labels(labels, m, "labels")
            correct = torch.zeros(2, dtype=torch.int64, device=features.device)
        _capi.check(_capi.lib.gm3d_linprobe_eval(_ptr(features), _ptr(labels), m, d, self.num_classes, _ptr(self.weight), _ptr(self.bias),
                                                 _ptr(self.running_mean), _ptr(self.running_var), None, _ptr(pred), _ptr(correct),
                                                 _stream()), "gm3d_linprobe_eval")
        return pred, correct

    def predict(self, features):
        """-> (m) int64 class indices: the largest logit, the smaller class on a tie."""
        return self._eval(features, None, True)[0]

    def score(self, features, labels):
        """top-1 accuracy (a fraction), counted on the device."""
        return float(self._eval(features, labels, False)[1][0].item()) / max(features.shape[0], 1)


def linear_probe(train_features, train_labels, test_features, test_labels, num_classes, weight=None, orders=None, **kwargs):
    """-> {"acc1", "acc5": of the last epoch, "max_acc1": the best top-1 over the evaluated epochs, "history"}: what main_linprob.py
    prints.  kwargs: LinearProbe's."""
    probe = LinearProbe(num_classes, **kwargs).fit(train_features, train_labels, test_features, test_labels, weight=weight, orders=orders)
    acc1, acc5 = probe.history[-1]
    return {"acc1": acc1, "acc5": acc5, "max_acc1": max(h[0] for h in probe.history), "history": probe.history}

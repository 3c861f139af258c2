"""Linear SVM on the MI355X: the solver of sklearn's SVC(C=0.01, kernel="linear") used by the pretraining validation
(validate.evaluate_svm), with the features kept on the device.

libsvm's C-SVC one-vs-one, without its shrinking heuristic (which does not move the fixed point): the f64 Gram matrix of the
class-grouped training rows (gm3d_svm_gram), one SMO workgroup per class pair (gm3d_svm_smo), the per-pair weight vectors
(gm3d_svm_weights) and the one-vs-one vote (gm3d_svm_predict).  The contracts are in include/gm3d.h.  The attributes follow
sklearn's names and pair order, so a fit can be held against SVC: classes_ (sorted unique labels), coef_ (P,d) f64, intercept_ (P,)
f64, n_iter_ (P,) int32 -- with sklearn's sign flip of coef_ / intercept_ for two classes.
"""
import ctypes

import numpy as np
import torch

from . import _capi
from .ops import _ptr, _stream

MAX_N, MAX_D, MAX_CLASSES, MAX_PAIR_ROWS = 16384, 1024, 64, 4096


def _require_cuda(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU path)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous %s tensor" % (name, dtype))


def _starts(class_start):
    cs = [int(v) for v in class_start]
    return (ctypes.c_int * len(cs))(*cs), len(cs) - 1


def pairs(ncls):
    """[(s, t)] in sklearn's (libsvm's) one-vs-one order."""
    return [(s, t) for s in range(ncls) for t in range(s + 1, ncls)]


def pair_offsets(class_start):
    """Offset of every pair's alpha in the concatenated alpha array, plus the total ((ncls-1) * n)."""
    cs = list(class_start)
    sizes = [cs[c + 1] - cs[c] for c in range(len(cs) - 1)]
    off = [0]
    for s, t in pairs(len(sizes)):
        off.append(off[-1] + sizes[s] + sizes[t])
    return off


def gram(X):
    """X (n,d) f32 CUDA -> K (n,n) f64 = X X^T (exactly symmetric)."""
    _require_cuda(X, torch.float32, "X")
    n, d = X.shape
    K = torch.empty(n, n, dtype=torch.float64, device=X.device)
    _capi.check(_capi.lib.gm3d_svm_gram(_ptr(X), n, d, _ptr(K), _stream()), "gm3d_svm_gram")
    return K


def smo(K, class_start, C=0.01, tol=1e-3, max_iter=0):
    """K (n,n) f64 of class-grouped rows, class_start (ncls+1) host ints -> alpha ((ncls-1)*n) f64, rho (P) f64, iters (P) int32,
    capped (1) int32 (pairs that reached the iteration cap)."""
    _require_cuda(K, torch.float64, "K")
    n = K.shape[0]
    cs, ncls = _starts(class_start)
    P = ncls * (ncls - 1) // 2
    dev = K.device
    alpha = torch.empty(max(ncls - 1, 0) * n, dtype=torch.float64, device=dev)
    rho = torch.empty(P, dtype=torch.float64, device=dev)
    iters = torch.empty(P, dtype=torch.int32, device=dev)
    capped = torch.zeros(1, dtype=torch.int32, device=dev)
    _capi.check(_capi.lib.gm3d_svm_smo(_ptr(K), n, ncls, cs, float(C), float(tol), int(max_iter), _ptr(alpha), _ptr(rho),
                                       _ptr(iters), _ptr(capped), _stream()), "gm3d_svm_smo")
    return alpha, rho, iters, capped


def weights(X, class_start, alpha):
    """w (P,d) f64, w_p = sum of y alpha x over the pair's rows (X the class-grouped rows the Gram was built from)."""
    _require_cuda(X, torch.float32, "X")
    _require_cuda(alpha, torch.float64, "alpha")
    n, d = X.shape
    cs, ncls = _starts(class_start)
    w = torch.empty(ncls * (ncls - 1) // 2, d, dtype=torch.float64, device=X.device)
    _capi.check(_capi.lib.gm3d_svm_weights(_ptr(X), n, d, ncls, cs, _ptr(alpha), _ptr(w), _stream()), "gm3d_svm_weights")
    return w


def vote(X, w, rho, ncls, labels=None):
    """X (m,d) f32 -> (pred (m) int64 class indices, correct (1) int64 or None); labels (m) int64 class indices, or None."""
    _require_cuda(X, torch.float32, "X")
    m, d = X.shape
    pred = torch.empty(m, dtype=torch.int64, device=X.device)
    correct = None
    if labels is not None:
        _require_cuda(labels, torch.int64, "labels")
        correct = torch.zeros(1, dtype=torch.int64, device=X.device)
    _capi.check(_capi.lib.gm3d_svm_predict(_ptr(X), m, d, ncls, _ptr(w), _ptr(rho), _ptr(labels), _ptr(pred), _ptr(correct),
                                           _stream()), "gm3d_svm_predict")
    return pred, correct


class LinearSVC:
    """SVC(C, kernel="linear") on CUDA tensors, solved on the device.  fit() synchronises once for the class counts."""

    def __init__(self, C=0.01, tol=1e-3, max_iter=0):
        self.C, self.tol, self.max_iter = C, tol, max_iter

    def fit(self, features, labels):
        X = features.detach().float().contiguous()
        _require_cuda(X, torch.float32, "features")
        y = labels.detach().to(X.device).view(-1)
        if y.numel() != X.shape[0]:
            raise ValueError("features and labels disagree: %d vs %d rows" % (X.shape[0], y.numel()))
        classes, inv, counts = torch.unique(y, sorted=True, return_inverse=True, return_counts=True)
        counts = counts.tolist()                                           # the one host synchronisation
        if len(counts) < 2:
            raise ValueError("the SVM needs at least two classes, got %d" % len(counts))
        self.classes_ = classes
        self.class_start_ = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64).tolist()
        order = torch.argsort(inv, stable=True)                            # class-grouped, dataset order inside a class
        Xg = X.index_select(0, order).contiguous()
        K = gram(Xg)
        alpha, rho, iters, capped = smo(K, self.class_start_, self.C, self.tol, self.max_iter)
        del K
        n_capped = int(capped.item())
        if n_capped:
            raise RuntimeError("LinearSVC: %d class pair(s) reached the iteration cap without converging" % n_capped)
        self.alpha_, self.rho_, self.n_iter_ = alpha, rho, iters
        self.w_ = weights(Xg, self.class_start_, alpha)
        sign = -1.0 if len(counts) == 2 else 1.0                           # sklearn flips the binary problem's sign
        self.coef_ = self.w_ * sign
        self.intercept_ = -rho * sign
        return self

    def _class_index(self, labels):
        lab = labels.to(self.classes_.device).view(-1)
        idx = torch.searchsorted(self.classes_, lab)
        idx = idx.clamp_(max=self.classes_.numel() - 1)
        return torch.where(self.classes_[idx] == lab, idx, torch.full_like(idx, -1)).to(torch.int64).contiguous()

    def predict_index(self, features, labels=None):
        """-> (class indices (m) int64, number of correct predictions (1) int64 or None)."""
        X = features.detach().float().contiguous()
        lab = self._class_index(labels) if labels is not None else None
        return vote(X, self.w_, self.rho_, self.classes_.numel(), lab)

    def predict(self, features):
        return self.classes_[self.predict_index(features)[0]]

    def score(self, features, labels):
        """accuracy, counted on the device."""
        _, correct = self.predict_index(features, labels)
        return float(correct.item()) / max(features.shape[0], 1)

"""Temperature-weighted k-NN probe of pretrained features on the MI355X: knn_classifier of Point-MAE_SA3D/main_knn.py:153-198,
the solver-free quality signal beside the linear SVM (validate.evaluate_knn).

One launch per (k, T): cosine similarities of L2-normalised rows on the exact-fp32 MFMA, an exact top-k by the strict total order
(similarity descending, training row ascending), exp(sim / T) votes summed per class in neighbour order, classes ranked by
(score descending, class ascending), top-1 / top-5 counted on the device.  No similarity matrix in memory, no host read before the
two final counters, bitwise reproducible.  The contracts are in include/gm3d.h; there is no CPU path.
"""
import torch

from . import _capi
from .ops import _ptr, _stream

MAX_N, MAX_D, MAX_K, MAX_CLASSES, D_MULTIPLE, MIN_D = 16384, 1024, 256, 64, 8, 8


def _require_cuda(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor (there is no CPU path)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError("%s must be a contiguous %s tensor" % (name, dtype))


def _features(t, name):
    _require_cuda(t, torch.float32, name)
    if t.dim() != 2:
        raise ValueError("%s must be (rows, channels), got %s" % (name, tuple(t.shape)))


def _pair(train_features, test_features):
    _features(train_features, "train_features")
    _features(test_features, "test_features")
    if train_features.shape[1] != test_features.shape[1]:
        raise ValueError("train and test features disagree: %d vs %d channels" % (train_features.shape[1], test_features.shape[1]))


def normalize(x):
    """x (n,d) f32 CUDA -> x / max(||x||_2, 1e-12) by row: F.normalize(x, p=2, dim=1)."""
    _features(x, "x")
    n, d = x.shape
    y = torch.empty_like(x)
    _capi.check(_capi.lib.gm3d_knn_probe_normalize(_ptr(x), n, d, _ptr(y), _stream()), "gm3d_knn_probe_normalize")
    return y


def neighbours(train_features, test_features, k):
    """-> (idx (m,k) int32, sim (m,k) f32): the k training rows of largest dot product for every test row, ordered by
    (similarity descending, training row ascending)."""
    _pair(train_features, test_features)
    (n, d), m = train_features.shape, test_features.shape[0]
    idx = torch.empty(m, k, dtype=torch.int32, device=train_features.device)
    sim = torch.empty(m, k, dtype=torch.float32, device=train_features.device)
    _capi.check(_capi.lib.gm3d_knn_probe_neighbours(_ptr(train_features), _ptr(test_features), n, m, d, int(k), _ptr(idx), _ptr(sim),
                                                    _stream()), "gm3d_knn_probe_neighbours")
    return idx, sim


def classify(train_features, train_labels, test_features, k, T, num_classes, test_labels=None, correct=None, return_probs=False):
    """One launch, nothing read back.  -> (top5 (m,5) int64, probs (m,num_classes) f32 or None, correct (2) int64 or None).
    `correct` (top-1, top-5 counts) is accumulated into (+=) when given, created zeroed when test_labels is given without it.
    Labels are class indices 0..num_classes-1 (the caller checks the range: knn_classifier does)."""
    _pair(train_features, test_features)
    _require_cuda(train_labels, torch.int64, "train_labels")
    (n, d), m = train_features.shape, test_features.shape[0]
    if train_labels.numel() != n:
        raise ValueError("train features and labels disagree: %d vs %d rows" % (n, train_labels.numel()))
    dev = train_features.device
    if test_labels is not None:
        _require_cuda(test_labels, torch.int64, "test_labels")
        if test_labels.numel() != m:
            raise ValueError("test features and labels disagree: %d vs %d rows" % (m, test_labels.numel()))
        if correct is None:
            correct = torch.zeros(2, dtype=torch.int64, device=dev)
        else:
            _require_cuda(correct, torch.int64, "correct")
            if correct.numel() != 2:
                raise ValueError("correct must hold two counters")
    top5 = torch.empty(m, 5, dtype=torch.int64, device=dev)
    probs = torch.empty(m, num_classes, dtype=torch.float32, device=dev) if return_probs else None
    _capi.check(_capi.lib.gm3d_knn_probe_classify(_ptr(train_features), _ptr(test_features), n, m, d, int(k), _ptr(train_labels),
                                                  int(num_classes), float(T), _ptr(test_labels), _ptr(top5), _ptr(probs),
                                                  _ptr(correct) if test_labels is not None else None, _stream()),
                "gm3d_knn_probe_classify")
    return top5, probs, (correct if test_labels is not None else None)


def knn_classifier(train_features, train_labels, test_features, test_labels, k, T, num_classes=None):
    """main_knn.py::knn_classifier: (top-1 %, top-5 %) of the weighted k-NN vote.  Features are already L2-normalised
    (main_knn.py:339-343; `normalize`), labels are class indices.  num_classes None: max label + 1 (one more host read).
    One launch, then one read of the two int64 counters."""
    _pair(train_features, test_features)
    train_labels = train_labels.view(-1)
    test_labels = test_labels.view(-1)
    _require_cuda(train_labels, torch.int64, "train_labels")
    _require_cuda(test_labels, torch.int64, "test_labels")
    lo = torch.minimum(train_labels.min(), test_labels.min()) if test_labels.numel() else train_labels.min()
    hi = torch.maximum(train_labels.max(), test_labels.max()) if test_labels.numel() else train_labels.max()
    if num_classes is None:
        lo_v, hi_v = torch.stack([lo, hi]).tolist()
        if lo_v < 0:
            raise ValueError("negative label %d" % lo_v)
        num_classes = max(hi_v + 1, 2)
        bad = None
    else:
        bad = (lo < 0) | (hi >= num_classes)       # stays on the device: read with the counters
    m = test_features.shape[0]
    _, _, correct = classify(train_features, train_labels, test_features, k, T, num_classes, test_labels)
    out = (torch.cat([correct, bad.view(1).to(torch.int64)]) if bad is not None else correct).tolist()   # the one read
    if bad is not None and out[2]:
        raise ValueError("labels outside 0..%d" % (num_classes - 1))
    total = max(m, 1)
    return out[0] * 100.0 / total, out[1] * 100.0 / total

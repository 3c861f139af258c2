"""Linear-SVM validation of the pretrained encoder: the reference's only quality signal during pretraining.

Mirror of P/main_pretrain_multi_gpu.py::validate / evaluate_svm (:414-483), P/utils/miscc.py::fps (:13-20) and
P/utils/dist_utils.py::gather_tensor (:50-54), SURVEY.md 8(f).1:
    points (B,8192,3) --FPS--> (B,1024,3) --model(points, all-False mask, noaug=True)--> (B,64,384)
    pooled = mean over tokens + max over tokens  -> all ranks gathered -> sklearn SVC(C=0.01, kernel='linear') on the CPU.
Differences of execution only: FPS emits the sampled points in the same launch (no separate gather), and the token
features are pooled on the GPU BEFORE the all-gather (the SVM never sees the un-pooled tokens), which cuts the
collective from 64x384 to 384 floats per cloud.

probe="knn" / "both" adds the reference's solver-free second probe, the temperature-weighted k-NN vote (evaluate_knn,
gm3d_amd.knn_probe), on the same gathered features.

svm_backend="hip" solves the same SVC(C=0.01, kernel='linear') problem on the GPU (gm3d_amd.svm.LinearSVC): the gathered,
pooled features never leave the device.  The default stays sklearn.

Point-M2AE (gm3d_amd.point_m2ae.PointM2AE) is validated the same way with its own input size: FPS to 2048 points
(Point-M2AE_SA3D/cfgs/config_Point_M2AE.yaml, npoints: 2048), then model(points, None, noaug=True), the final-normed
coarsest tokens (B,64,384), pooled to mean + max.  That feature is stated, not pinned: the reference ships no Point-M2AE
source (point_m2ae.py).
"""
import numpy as np
import torch
import torch.distributed as dist

from . import ops


def fps(data, number):
    """miscc.fps: data (B,N,3) -> the `number` farthest-point samples (B,number,3), in sampling order."""
    return ops.fps(data.contiguous().float(), number)[1]


MAE_NPOINTS, M2AE_NPOINTS = 1024, 2048


def _is_m2ae(raw):
    from .point_m2ae import PointM2AE
    return isinstance(raw, PointM2AE)


def default_npoints(model):
    """The validation input size of the model: 2048 points for Point-M2AE, 1024 (the Point-MAE value) otherwise."""
    raw = model.module if hasattr(model, "module") else model
    return M2AE_NPOINTS if _is_m2ae(raw) else MAE_NPOINTS


@torch.no_grad()
def extract_features(model, points, npoints=None, bf16=False):
    """-> token features (B,64,384) of the eval-mode encoder (P/:427-433).  npoints None: default_npoints(model)."""
    raw = model.module if hasattr(model, "module") else model
    if npoints is None:
        npoints = default_npoints(raw)
    pts = fps(points, npoints)      # the reference resamples unconditionally (P/main_pretrain_multi_gpu.py:430)
    assert pts.size(1) == npoints
    if _is_m2ae(raw):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            return raw(pts, None, noaug=True).float()
    mask = torch.zeros(pts.shape[0], raw.num_group, dtype=torch.bool, device=pts.device)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        return raw(pts, mask, noaug=True, num_visible=raw.num_group).float()


def pool_features(features):
    """(B,T,C) -> (B,C): mean(1) + max(1), the SVM input of evaluate_svm (:479,481)."""
    return features.mean(1) + features.max(1)[0]


def gather_tensor(tensor, world_size=None):
    """dist_utils.gather_tensor: all_gather + concat along dim 0 (identity without a process group)."""
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return tensor
    outs = [torch.empty_like(tensor) for _ in range(dist.get_world_size())]
    dist.all_gather(outs, tensor.contiguous())
    return torch.cat(outs, dim=0)


def evaluate_svm(train_features, train_labels, test_features, test_labels, backend="sklearn"):
    """P/:476-483.  Accepts token features (n,T,C) like the reference or already pooled (n,C).
    backend "sklearn": SVC on the host (numpy or CPU inputs); "hip": gm3d_amd.svm.LinearSVC on the GPU (CUDA tensors stay there)."""
    if backend == "hip":
        return _evaluate_svm_hip(train_features, train_labels, test_features, test_labels)
    if backend != "sklearn":
        raise ValueError("unknown SVM backend %r (sklearn or hip)" % (backend,))
    from sklearn.svm import SVC
    def pooled(f):
        f = np.asarray(f)
        return f.mean(1) + f.max(1) if f.ndim == 3 else f
    clf = SVC(C=0.01, kernel="linear")
    clf.fit(pooled(train_features), np.asarray(train_labels))
    pred = clf.predict(pooled(test_features))
    return np.sum(np.asarray(test_labels) == pred) * 1.0 / pred.shape[0]


def _evaluate_svm_hip(train_features, train_labels, test_features, test_labels):
    from .svm import LinearSVC

    def dev(t, dtype):
        t = torch.as_tensor(t)
        return (t if t.is_cuda else t.to("cuda")).to(dtype)

    def pooled(f):
        f = dev(f, torch.float32)
        return pool_features(f) if f.dim() == 3 else f
    clf = LinearSVC(C=0.01).fit(pooled(train_features), dev(train_labels, torch.int64))
    return clf.score(pooled(test_features), dev(test_labels, torch.int64))


def evaluate_knn(train_features, train_labels, test_features, test_labels, ks=(10, 20, 100, 200), T=0.07):
    """The reference's second probe (Point-MAE_SA3D/main_knn.py:339-363): the temperature-weighted k-NN vote on L2-normalised
    features, on the GPU (gm3d_amd.knn_probe).  Accepts token features (n,T,C) or already pooled (n,C), pooled as evaluate_svm pools;
    labels are class indices.  -> {k: (top-1 %, top-5 %)}; a k above the number of training rows is skipped with a warning."""
    import warnings
    from . import knn_probe

    def dev(t, dtype):
        t = torch.as_tensor(t)
        return (t if t.is_cuda else t.to("cuda")).to(dtype)

    def prepared(f):
        f = dev(f, torch.float32)
        return knn_probe.normalize((pool_features(f) if f.dim() == 3 else f).contiguous())
    xtr, xte = prepared(train_features), prepared(test_features)
    ytr, yte = dev(train_labels, torch.int64).view(-1).contiguous(), dev(test_labels, torch.int64).view(-1).contiguous()
    num_classes = max(int(torch.maximum(ytr.max(), yte.max()).item()) + 1, 2)
    out = {}
    for k in ks:
        if k > xtr.shape[0]:
            warnings.warn("evaluate_knn: k = %d skipped, only %d training rows" % (k, xtr.shape[0]))
            continue
        out[k] = knn_probe.knn_classifier(xtr, ytr, xte, yte, k, T, num_classes)
    return out


def evaluate_linear(train_features, train_labels, test_features, test_labels, num_classes=None, **probe_kwargs):
    """The reference's third probe (Point-MAE_SA3D/main_linprob.py:219-263): BatchNorm1d(affine=False) + Linear trained with SGD on
    the frozen features, on the GPU (gm3d_amd.linear_probe).  Accepts token features (n,T,C) or already pooled (n,C), pooled as
    evaluate_svm pools; labels are class indices.  num_classes None: max label + 1 (one more host read).  probe_kwargs:
    LinearProbe's (batch_size, epochs, ...) and fit's weight / orders; a batch_size above the training rows is lowered to them.
    -> {"acc1", "acc5", "max_acc1", "history"}, in percent."""
    from . import linear_probe

    def dev(t, dtype):
        t = torch.as_tensor(t)
        return (t if t.is_cuda else t.to("cuda")).to(dtype)

    def pooled(f):
        f = dev(f, torch.float32)
        return (pool_features(f) if f.dim() == 3 else f).contiguous()
    xtr, xte = pooled(train_features), pooled(test_features)
    ytr, yte = dev(train_labels, torch.int64).view(-1).contiguous(), dev(test_labels, torch.int64).view(-1).contiguous()
    if num_classes is None:
        num_classes = max(int(torch.maximum(ytr.max(), yte.max()).item()) + 1, 2)
    probe_kwargs["batch_size"] = min(probe_kwargs.get("batch_size", 512), xtr.shape[0])
    return linear_probe.linear_probe(xtr, ytr, xte, yte, num_classes, **probe_kwargs)


@torch.no_grad()
def validate(model, extra_train_dataloader, test_dataloader, npoints=None, device="cuda", bf16=False, svm_backend="sklearn",
             probe="svm", knn_ks=(10, 20, 100, 200), knn_T=0.07, linear_kwargs=None):
    """Loaders yield (taxonomy_ids, model_ids, (points, label)) like the reference's ModelNet loaders (:428-431).
    Returns the SVM accuracy (computed on every rank from the gathered features, like the reference).  npoints None:
    default_npoints(model).  svm_backend "hip" keeps the gathered features on the GPU and solves there.
    probe "svm" (default): the SVM accuracy; "knn": evaluate_knn's {k: (top-1 %, top-5 %)} on the same gathered features, no SVM;
    "both": (SVM accuracy, that dict); "linear": evaluate_linear's dict (linear_kwargs: its keyword arguments), no SVM;
    "all": (SVM accuracy, the k-NN dict, the linear dict)."""
    if svm_backend not in ("sklearn", "hip"):
        raise ValueError("unknown SVM backend %r (sklearn or hip)" % (svm_backend,))
    if probe not in ("svm", "knn", "both", "linear", "all"):
        raise ValueError("unknown probe %r (svm, knn, both, linear or all)" % (probe,))
    was_training = model.training
    model.eval()
    feats = {}
    for split, loader in (("train", extra_train_dataloader), ("test", test_dataloader)):
        f, l = [], []
        for _, _, data in loader:
            points, label = data[0].to(device), data[1].to(device)
            f.append(pool_features(extract_features(model, points, npoints, bf16=bf16)))
            l.append(label.view(-1))
        feats[split] = (gather_tensor(torch.cat(f, 0)), gather_tensor(torch.cat(l, 0)))
    model.train(was_training)
    knn = linear = None
    if probe in ("linear", "all"):
        linear = evaluate_linear(feats["train"][0], feats["train"][1], feats["test"][0], feats["test"][1], **(linear_kwargs or {}))
        if probe == "linear":
            return linear
    if probe != "svm":
        knn = evaluate_knn(feats["train"][0], feats["train"][1], feats["test"][0], feats["test"][1], ks=knn_ks, T=knn_T)
        if probe == "knn":
            return knn
    if svm_backend == "hip":
        acc = evaluate_svm(feats["train"][0], feats["train"][1], feats["test"][0], feats["test"][1], backend="hip")
    else:
        acc = evaluate_svm(feats["train"][0].cpu().numpy(), feats["train"][1].cpu().numpy(),
                           feats["test"][0].cpu().numpy(), feats["test"][1].cpu().numpy())
    if probe == "all":
        return acc, knn, linear
    return acc if probe == "svm" else (acc, knn)

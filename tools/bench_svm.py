"""Linear-SVM validation: sklearn's SVC(C=0.01, kernel="linear") on the host against gm3d_amd.svm.LinearSVC on the GPU.

Default: synthetic ModelNet40-shaped features (9,843 train / 2,468 test clouds, 40 classes with ModelNet40's class counts, 384-wide,
fixed seed).  Prints, per backend, fit and predict wall times over --repeats runs (median, min, max), the GPU time of every stage
from HIP events (Gram, SMO, weights, vote), the iteration counts, and the prediction agreement.

--model mae|m2ae: instead, the whole validate() on synthetic labelled 8192-point clouds (--train / --test clouds, random-init model,
batch --batch) under both backends, wall time per run.

Prints one JSON line at the end.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import svm_ref  # noqa: E402  (the synthetic ModelNet40-shaped features)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def bench_features(repeats, sk_repeats):
    from sklearn.svm import SVC

    from gm3d_amd import svm
    Xtr, ytr, Xte, yte = svm_ref.modelnet40_like(seed=0)
    res = {"shape": {"train": len(ytr), "test": len(yte), "classes": 40, "d": Xtr.shape[1]}}

    fit_t, pred_t = [], []
    for _ in range(sk_repeats):
        t0 = time.perf_counter()
        clf = SVC(C=0.01, kernel="linear").fit(Xtr.astype(np.float64), ytr)
        t1 = time.perf_counter()
        ref = clf.predict(Xte.astype(np.float64))
        t2 = time.perf_counter()
        fit_t.append(t1 - t0)
        pred_t.append(t2 - t1)
    res["sklearn"] = {"fit_s": spread(fit_t), "predict_s": spread(pred_t), "acc": float((ref == yte).mean()),
                      "n_iter": [int(clf.n_iter_.min()), int(clf.n_iter_.max())]}

    X, y = torch.from_numpy(Xtr).cuda(), torch.from_numpy(ytr).cuda()
    T, yt = torch.from_numpy(Xte).cuda(), torch.from_numpy(yte).cuda()
    svm.LinearSVC().fit(X, y).predict(T)                  # warm-up: module load, LDS attribute, allocator
    torch.cuda.synchronize()
    fit_t, pred_t, stages = [], [], {k: [] for k in ("gram", "smo", "weights", "vote")}
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ours = svm.LinearSVC().fit(X, y)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, correct = ours.predict_index(T, yt)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        fit_t.append(t1 - t0)
        pred_t.append(t2 - t1)
        # the same stages once more under events, on class-grouped rows
        Xg = X.index_select(0, torch.argsort(torch.searchsorted(ours.classes_, y), stable=True)).contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        K = svm.gram(Xg)
        ev[1].record()
        alpha, rho, _, _ = svm.smo(K, ours.class_start_)
        ev[2].record()
        w = svm.weights(Xg, ours.class_start_, alpha)
        ev[3].record()
        svm.vote(T, w, rho, 40)
        ev[4].record()
        torch.cuda.synchronize()
        for k, name in enumerate(stages):
            stages[name].append(ev[k].elapsed_time(ev[k + 1]) / 1e3)
        del K
    pred = ours.predict(T).cpu().numpy()
    it = ours.n_iter_.cpu().numpy()
    res["hip"] = {"fit_s": spread(fit_t), "predict_s": spread(pred_t), "acc": float(correct.item()) / len(yte),
                  "gpu_s": {k: spread(v) for k, v in stages.items()}, "n_iter": [int(it.min()), int(it.max())]}
    res["agreement"] = float((pred == ref).mean())
    res["coef_rel_err"] = float(np.abs(ours.coef_.cpu().numpy() - clf.coef_).max() / np.abs(clf.coef_).max())
    return res


class CloudLoader:
    """Re-iterable (None, None, (points (B,8192,3), label (B,))) batches made on the GPU: class c is an ellipsoid with its own
    axes plus noise.  Fixed seed per batch, so both backends see the same clouds."""

    def __init__(self, counts, batch, seed):
        self.labels = torch.from_numpy(np.random.RandomState(seed).permutation(np.repeat(np.arange(len(counts)), counts)))
        self.batch, self.seed = batch, seed
        c = torch.arange(len(counts), dtype=torch.float32)
        self.axes = torch.stack([1.0 + 0.0 * c, 0.3 + 0.7 * (c % 8) / 8, 0.3 + 0.7 * (c // 8) / 5], 1).cuda()

    def __iter__(self):
        for k, b0 in enumerate(range(0, len(self.labels), self.batch)):
            lab = self.labels[b0:b0 + self.batch].cuda()
            g = torch.Generator(device="cuda").manual_seed(self.seed * 100003 + k)
            d = torch.randn(len(lab), 8192, 3, device="cuda", generator=g)
            pts = d / d.norm(dim=-1, keepdim=True) * self.axes[lab][:, None, :]
            yield None, None, (pts + 0.05 * torch.randn(pts.shape, device="cuda", generator=g), lab)


def bench_validate(model_name, repeats, batch, n_train, n_test):
    from gm3d_amd import validate as V
    torch.manual_seed(0)
    if model_name == "mae":
        from gm3d_amd import models_mae_learn_loss as M
        model = M.mae_vit_base_patch16_dec512d8b().cuda()
    else:
        from gm3d_amd import point_m2ae as P
        model = P.PointM2AE().cuda()

    def scaled(counts, total):
        c = np.maximum(1, np.round(np.asarray(counts) * total / sum(counts))).astype(int)
        return c.tolist()
    train = CloudLoader(scaled(svm_ref.MODELNET40_TRAIN, n_train), batch, 1)
    test = CloudLoader(scaled(svm_ref.MODELNET40_TEST, n_test), batch, 2)
    res = {"model": model_name, "train": len(train.labels), "test": len(test.labels), "batch": batch,
           "npoints": V.default_npoints(model)}
    t0 = time.perf_counter()
    for _, _, (pts, _) in test:                          # warm-up of the extraction path
        V.extract_features(model.eval(), pts)
        break
    torch.cuda.synchronize()
    res["warmup_s"] = time.perf_counter() - t0
    # the extraction alone, then the whole validate() under each backend
    ext = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for loader in (train, test):
                for _, _, (pts, _) in loader:
                    V.pool_features(V.extract_features(model, pts))
        torch.cuda.synchronize()
        ext.append(time.perf_counter() - t0)
    res["extract_s"] = spread(ext)
    for backend in ("hip", "sklearn"):
        ts, accs = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            accs.append(float(V.validate(model, train, test, svm_backend=backend)))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[backend] = {"validate_s": spread(ts), "acc": accs[-1]}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", choices=("mae", "m2ae"), default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sk-repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--train", type=int, default=9843)
    ap.add_argument("--test", type=int, default=2468)
    args = ap.parse_args()
    if args.model is None:
        res = bench_features(args.repeats, args.sk_repeats)
        print("sklearn fit %.2f s (%.2f-%.2f), predict %.2f s; acc %.4f" % (
            res["sklearn"]["fit_s"]["median"], res["sklearn"]["fit_s"]["min"], res["sklearn"]["fit_s"]["max"],
            res["sklearn"]["predict_s"]["median"], res["sklearn"]["acc"]))
        h = res["hip"]
        print("hip     fit %.4f s (%.4f-%.4f), predict %.5f s; acc %.4f; gpu: %s" % (
            h["fit_s"]["median"], h["fit_s"]["min"], h["fit_s"]["max"], h["predict_s"]["median"], h["acc"],
            ", ".join("%s %.2f ms" % (k, v["median"] * 1e3) for k, v in h["gpu_s"].items())))
        print("agreement %.4f, coef rel err %.2e, iterations hip %s sklearn %s" % (
            res["agreement"], res["coef_rel_err"], h["n_iter"], res["sklearn"]["n_iter"]))
    else:
        res = bench_validate(args.model, args.repeats, args.batch, args.train, args.test)
        print("%s: %d/%d clouds, npoints %d; extraction %.2f s; validate hip %.2f s (acc %.4f), sklearn %.2f s (acc %.4f)" % (
            res["model"], res["train"], res["test"], res["npoints"], res["extract_s"]["median"], res["hip"]["validate_s"]["median"],
            res["hip"]["acc"], res["sklearn"]["validate_s"]["median"], res["sklearn"]["acc"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Weighted k-NN probe: gm3d_amd.knn_probe.knn_classifier (one launch) beside the aten chain that restates the reference on the same
GPU (mm + topk + gather / scatter_ + sort, 500 chunks with two host reads each, main_knn.py:153-198).

Synthetic ModelNet40-shaped features (9,843 train / 2,468 test rows, 40 classes, 384-wide, fixed seed), L2-normalised; k = 20 and
200, T = 0.07.  Per k: wall time of --repeats runs of each (median, min, max; one warm-up before), the GPU time of the launch from
HIP events, and both results.  Writes profiles/knn_probe_bench.json and prints it as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import svm_ref  # noqa: E402  (the synthetic ModelNet40-shaped features)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def aten_chain(train_features, train_labels, test_features, test_labels, k, T, num_classes, num_chunks=500):
    """The reference's sequence of aten calls, chunk for chunk."""
    top1, top5, total = 0.0, 0.0, 0
    train_t = train_features.t()
    m = test_labels.shape[0]
    per_chunk = max(m // num_chunks, 1)
    one_hot = torch.zeros(k, num_classes, device=train_features.device)
    for i in range(0, m, per_chunk):
        feats, targets = test_features[i:i + per_chunk], test_labels[i:i + per_chunk]
        b = targets.shape[0]
        sim, idx = torch.mm(feats, train_t).topk(k, largest=True, sorted=True)
        retrieved = torch.gather(train_labels.view(1, -1).expand(b, -1), 1, idx)
        one_hot.resize_(b * k, num_classes).zero_()
        one_hot.scatter_(1, retrieved.view(-1, 1), 1)
        w = sim.clone().div_(T).exp_()
        probs = torch.sum(one_hot.view(b, -1, num_classes) * w.view(b, -1, 1), 1)
        _, pred = probs.sort(1, True)
        correct = pred.eq(targets.view(-1, 1))
        top1 += correct.narrow(1, 0, 1).sum().item()
        top5 += correct.narrow(1, 0, min(5, k)).sum().item()
        total += b
    return top1 * 100.0 / total, top5 * 100.0 / total


def timed(fn, repeats):
    out = fn()                                             # warm-up: module load, LDS attribute, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return spread(ts), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_probe_bench.json"))
    args = ap.parse_args()
    from gm3d_amd import knn_probe as KP
    Xtr, ytr, Xte, yte = svm_ref.modelnet40_like(seed=0)
    xtr, xte = KP.normalize(torch.from_numpy(Xtr).cuda()), KP.normalize(torch.from_numpy(Xte).cuda())
    ltr, lte = torch.from_numpy(ytr).cuda().long(), torch.from_numpy(yte).cuda().long()
    T = 0.07
    res = {"device": torch.cuda.get_device_name(0), "shape": {"train": len(ytr), "test": len(yte), "classes": 40, "d": Xtr.shape[1]},
           "T": T, "k": {}}
    for k in args.ks:
        hip_t, hip = timed(lambda: KP.knn_classifier(xtr, ltr, xte, lte, k, T, 40), args.repeats)
        ev = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            KP.classify(xtr, ltr, xte, k, T, 40, test_labels=lte)
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b) / 1e3)
        aten_t, aten = timed(lambda: aten_chain(xtr, ltr, xte, lte, k, T, 40), args.repeats)
        res["k"][str(k)] = {"hip_wall_s": hip_t, "hip_gpu_s": spread(ev), "aten_wall_s": aten_t, "hip_top": list(hip),
                            "aten_top": list(aten)}
        print("k = %3d: hip %.2f ms wall (%.2f-%.2f; launch %.2f ms on the GPU), aten chain %.1f ms (%.1f-%.1f); top-1/5 hip %s aten %s"
              % (k, hip_t["median"] * 1e3, hip_t["min"] * 1e3, hip_t["max"] * 1e3, statistics.median(ev) * 1e3,
                 aten_t["median"] * 1e3, aten_t["min"] * 1e3, aten_t["max"] * 1e3, list(hip), list(aten)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

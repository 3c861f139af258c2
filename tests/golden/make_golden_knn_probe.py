"""Regenerates tests/golden/knn_probe.npz: the reference's own knn_classifier run in place.

    python tests/golden/make_golden_knn_probe.py <path of the reference checkout>

The source of the function `knn_classifier` is read from <reference>/Point-MAE_SA3D/main_knn.py at generation time and executed
with torch alone (the module's top-level imports need timm / torchvision, which this needs not); nothing of it is stored.
Inputs: seeded, weakly clustered features, n = 1024 training rows, m = 512 test rows (the reference splits the test set into 500
chunks, so it needs m >= 500), d = 32, 10 classes, L2-normalised as main_knn.py:339-343 does; k = 10 and 20, T = 0.07.
The test rows are the first 512 of a larger seeded draw on which the float64 restatement (tests/knn_probe_ref.py) finds, for both
k, at least 5 voted classes, a similarity gap above 1e-4 at the k | k+1 boundary and relative score margins above 1e-3 at ranks
1|2 and 5|6: the stored top-1 / top-5 then do not depend on any tie rule or rounding, and the tests compare them for equality.
The generator asserts exactly that on what it stores."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import knn_probe_ref as KR  # noqa: E402

N, M, D, NCLS, KS, T, SEED, POOL = 1024, 512, 32, 10, (10, 20), 0.07, 0, 4096
MIN_VOTED, MIN_GAP, MIN_MARGIN = 5, 1e-4, 1e-3


def reference_function(root):
    path = os.path.join(root, "Point-MAE_SA3D", "main_knn.py")
    src = open(path).read()
    node = next(f for f in ast.parse(src).body if isinstance(f, ast.FunctionDef) and f.name == "knn_classifier")
    lines = src.splitlines()[node.lineno - 1:node.end_lineno]      # from `def`: the no_grad decorator is applied below
    env = {"torch": torch}
    exec(compile("\n".join(lines), path, "exec"), env)
    return torch.no_grad()(env["knn_classifier"])


def unambiguous(res):
    return (res["voted"] >= MIN_VOTED) & (res["gap"] > MIN_GAP) & (res["margin12"] > MIN_MARGIN) & (res["margin56"] > MIN_MARGIN)


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(NCLS, D, generator=g)
    ytr = torch.arange(N) % NCLS
    ypool = torch.arange(POOL) % NCLS
    xtr = 0.35 * centres[ytr] + torch.randn(N, D, generator=g)
    xpool = 0.35 * centres[ypool] + torch.randn(POOL, D, generator=g)
    xtr = torch.nn.functional.normalize(xtr, dim=1, p=2)
    xpool = torch.nn.functional.normalize(xpool, dim=1, p=2)
    keep = np.ones(POOL, bool)
    for k in KS:
        keep &= unambiguous(KR.knn_classifier(xtr.numpy(), ytr.numpy(), xpool.numpy(), ypool.numpy(), k, T, NCLS))
    rows = np.nonzero(keep)[0][:M]
    assert rows.size == M, "seed %d leaves only %d unambiguous test rows: change SEED" % (seed, rows.size)
    return xtr, ytr, xpool[rows].contiguous(), ypool[rows].contiguous()


def main(root):
    ref = reference_function(root)
    xtr, ytr, xte, yte = inputs(SEED)
    out = {"train": xtr.numpy(), "train_labels": ytr.numpy().astype(np.uint8), "test": xte.numpy(),
           "test_labels": yte.numpy().astype(np.uint8), "ks": np.array(KS, np.int32), "T": np.array(T, np.float64),
           "num_classes": np.array(NCLS, np.int32)}
    top = []
    for k in KS:
        res = KR.knn_classifier(xtr.numpy(), ytr.numpy(), xte.numpy(), yte.numpy(), k, T, NCLS)
        assert unambiguous(res).all()
        top1, top5 = ref(xtr, ytr, xte, yte, k, T, num_classes=NCLS)
        assert (top1, top5) == (res["top1"], res["top5"]), (k, top1, top5, res["top1"], res["top5"])
        top.append((top1, top5))
        print("k = %d: top1 %.4f top5 %.4f" % (k, top1, top5))
    out["top"] = np.array(top, np.float64)
    path = os.path.join(HERE, "knn_probe.npz")
    np.savez(path, **out)
    assert os.path.getsize(path) < 256 * 1000, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])

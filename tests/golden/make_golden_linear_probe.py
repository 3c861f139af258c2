"""Regenerates tests/golden/linear_probe.npz: the float64 linear probe under the reference's own learning-rate schedule.

    python tests/golden/make_golden_linear_probe.py <path of the reference checkout>

The source of the function `adjust_learning_rate` is read from <reference>/Point-MAE_SA3D/util/lr_sched.py at generation time and
executed; nothing of it is stored.  The probe (tests/linear_probe_ref.py: BatchNorm1d(affine=False, eps=1e-6) -> Linear, SGD with
momentum 0.9, cross-entropy) runs in float64 on seeded, weakly clustered features: n = 640, m = 256, d = 384, 40 classes, batch 100
(a dropped tail of 40 rows), 6 epochs, 2 warm-up epochs, peak rate 0.1 * 100 / 256, the rows in the sampler's order for seed 0, the
initial weights trunc_normal_(std=0.01) on a generator seeded 0.  The features have per-column scales 0.5 .. 2, an offset of +3 and
one all-zero column; they are regenerated from their seed by the tests (a sum of each is stored to notice a generator that changed).
The test rows are the first 256 of a pool of 1024 whose float64 logits keep a gap above 1e-3 at ranks 1|2 and 5|6 at every evaluated
epoch from the second on: the stored hit counts of those epochs depend on no rounding, and the tests compare them for equality.  The
generator asserts exactly that on what it stores."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import linear_probe_ref as LR  # noqa: E402


def reference_function(root):
    path = os.path.join(root, "Point-MAE_SA3D", "util", "lr_sched.py")
    src = open(path).read()
    node = next(f for f in ast.parse(src).body if isinstance(f, ast.FunctionDef) and f.name == "adjust_learning_rate")
    lines = src.splitlines()[node.lineno - 1:node.end_lineno]
    import math
    env = {"math": math}
    exec(compile("\n".join(lines), path, "exec"), env)
    return env["adjust_learning_rate"]


def main(root):
    f = LR.FIXTURE
    n, m, C, batch, E, warm = f["n"], f["m"], f["num_classes"], f["batch"], f["epochs"], f["warmup_epochs"]
    lr = LR.peak_lr(batch)
    rates = LR.learning_rates(E, n // batch, lr, 0.0, warm, adjust=reference_function(root))
    assert np.array_equal(rates, LR.learning_rates(E, n // batch, lr, 0.0, warm)), "the restated schedule differs from the reference's"
    X, y, Qpool, ypool, weight, orders = LR.fixture_inputs()
    rows = LR.select_rows(X, y, Qpool, ypool, m, C, weight, orders, batch, E, warm, lr, rates=rates)
    res = LR.fit(X, y, Qpool[rows], ypool[rows], C, weight, orders, batch, E, warm, lr, rates=rates)
    assert res["eval_epochs"] == list(range(1, E + 1))
    for e, gap in zip(res["eval_epochs"], res["min_gap"]):
        print("epoch %d: hits %s, smallest gaps 1|2 %.3e 5|6 %.3e" % (e, res["hits"][e - 1], gap[0], gap[1]))
        assert e < 2 or min(gap) > LR.MIN_GAP
    out = {"rates": rates, "rows": rows.astype(np.int32), "hits": np.array(res["hits"], np.int64),
           "min_gap": np.array(res["min_gap"], np.float64), "x_sum": np.array([X.astype(np.float64).sum(), Qpool.astype(np.float64).sum()]),
           "w0_sum": np.array(weight.astype(np.float64).sum())}
    for k in LR.TENSORS:
        out[k] = res[k]
    path = os.path.join(HERE, "linear_probe.npz")
    np.savez(path, **out)
    assert os.path.getsize(path) < 256 * 1000, os.path.getsize(path)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main(sys.argv[1])

"""CPU: the weighted k-NN probe (include/gm3d.h, gm3d_amd/csrc/knn_probe.hip, gm3d_amd/knn_probe.py).  The float64 restatement the
GPU tests trust (tests/knn_probe_ref.py) reproduces the reference's own top-1 / top-5 of the committed fixture exactly; the entry
points refuse every shape outside their contract on the host; the header states the limits the wrapper carries."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import knn_probe_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)      # 16-byte aligned, never dereferenced: the shape check fails (or the empty batch returns) first


def _lib():
    from gm3d_amd._capi import lib
    return lib


def _nb(n=100, m=10, d=64, k=5, X=ONE, Q=ONE, idx=ONE, sim=ONE):
    return _lib().gm3d_knn_probe_neighbours(X, Q, n, m, d, k, idx, sim, None)


def _cl(n=100, m=10, d=64, k=5, ncls=10, T=0.07, X=ONE, Q=ONE, lab=ONE, tlab=None, top5=ONE, correct=None):
    return _lib().gm3d_knn_probe_classify(X, Q, n, m, d, k, lab, ncls, T, tlab, top5, None, correct, None)


def test_restatement_reproduces_the_reference_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "knn_probe.npz"))
    assert z["train"].shape == (1024, 32) and z["test"].shape == (512, 32)
    for k, (top1, top5) in zip(z["ks"].tolist(), z["top"].tolist()):
        res = KR.knn_classifier(z["train"], z["train_labels"].astype(np.int64), z["test"], z["test_labels"].astype(np.int64), k,
                                float(z["T"]), int(z["num_classes"]))
        assert (res["top1"], res["top5"]) == (top1, top5)
        # the fixture is unambiguous: no tie rule or rounding can move it
        assert res["voted"].min() >= 5 and res["gap"].min() > 1e-4
        assert res["margin12"].min() > 1e-3 and res["margin56"].min() > 1e-3


def test_restatement_tie_rules():
    X = np.ones((7, 8), np.float32)
    idx, sim, gap = KR.neighbours(X, X[:2], 3)
    assert np.array_equal(idx, [[0, 1, 2]] * 2) and np.all(gap == 0)
    res = KR.knn_classifier(X, np.array([3, 3, 1, 1, 0, 0, 0]), X[:2], np.array([1, 0]), 4, 0.07, 5)
    assert np.array_equal(res["ranking"][0], [1, 3, 0, 2, 4])         # equal scores by class id, the unvoted classes after
    assert res["top1"] == 50.0 and res["top5"] == 100.0


def test_entry_points_refuse_shapes_outside_the_contract():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_OK
    lib = _lib()
    for call in (_nb, _cl):
        assert call(n=0) == GM3D_EINVAL
        assert call(n=16385) == GM3D_EUNSUPPORTED
        assert call(m=-1) == GM3D_EINVAL
        assert call(d=0) == GM3D_EINVAL
        assert call(d=4) == GM3D_EUNSUPPORTED                          # below 8
        assert call(d=100) == GM3D_EUNSUPPORTED                        # not a multiple of 8
        assert call(d=1032) == GM3D_EUNSUPPORTED
        assert call(k=0) == GM3D_EINVAL
        assert call(n=100, k=101) == GM3D_EINVAL                       # k > n
        assert call(n=1000, k=257) == GM3D_EUNSUPPORTED
        assert call(X=None) == GM3D_EINVAL
        assert call(Q=None) == GM3D_EINVAL
        assert call(X=ctypes.c_void_p(20)) == GM3D_EINVAL              # not 16-byte aligned
        # m == 0 launches nothing, at every accepted limit
        assert call(m=0) == GM3D_OK
        assert call(n=16384, m=0, d=1024, k=256) == GM3D_OK
        assert call(n=1, m=0, d=8, k=1) == GM3D_OK
        # the last accepted value of each limit passes the shape checks: a NULL data pointer fails after them
        assert call(n=16384, d=1024, k=256, X=None) == GM3D_EINVAL
        assert call(n=1, d=8, k=1, X=None) == GM3D_EINVAL
    assert _nb(idx=None) == GM3D_EINVAL
    assert _nb(sim=None) == GM3D_EINVAL
    assert _cl(ncls=0) == GM3D_EINVAL
    assert _cl(ncls=1) == GM3D_EUNSUPPORTED
    assert _cl(ncls=65) == GM3D_EUNSUPPORTED
    assert _cl(T=0.0) == GM3D_EINVAL
    assert _cl(T=-1.0) == GM3D_EINVAL
    assert _cl(T=float("nan")) == GM3D_EINVAL
    assert _cl(lab=None) == GM3D_EINVAL
    assert _cl(top5=None) == GM3D_EINVAL
    assert _cl(tlab=ONE, correct=None) == GM3D_EINVAL                  # labels without counters
    assert _cl(m=0, ncls=64) == GM3D_OK and _cl(m=0, ncls=2) == GM3D_OK
    assert _cl(m=0, ncls=65) == GM3D_EUNSUPPORTED                      # the shape is checked before the empty batch returns
    # normalize: any n >= 0, d >= 1
    assert lib.gm3d_knn_probe_normalize(ONE, -1, 8, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_knn_probe_normalize(ONE, 4, 0, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_knn_probe_normalize(None, 4, 8, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_knn_probe_normalize(ONE, 4, 8, None, None) == GM3D_EINVAL
    assert lib.gm3d_knn_probe_normalize(None, 0, 8, None, None) == GM3D_OK


def test_header_states_the_limits_of_the_wrapper():
    from gm3d_amd import knn_probe as KP
    txt = open(os.path.join(ROOT, "include", "gm3d.h")).read()
    sec = txt[txt.index("Weighted k-NN probe"):]
    sec = sec[:sec.index("int gm3d_knn_probe_normalize")]
    line = re.search(r"1 <= n <= (\d+), (\d+) <= d <= (\d+), d % (\d+) == 0, 1 <= k <= min\(n, (\d+)\), 2 <= ncls <= (\d+), T > 0, m >= 0",
                     sec)
    assert line, "the limits line of the k-NN probe section"
    assert tuple(int(v) for v in line.groups()) == (KP.MAX_N, KP.MIN_D, KP.MAX_D, KP.D_MULTIPLE, KP.MAX_K, KP.MAX_CLASSES)
    src = open(os.path.join(ROOT, "gm3d_amd", "csrc", "knn_probe.hip")).read()
    consts = re.search(r"KP_MAX_N = (\d+), KP_MAX_D = (\d+), KP_MAX_K = (\d+), KP_MAX_CLS = (\d+);", src)
    assert tuple(int(v) for v in consts.groups()) == (KP.MAX_N, KP.MAX_D, KP.MAX_K, KP.MAX_CLASSES)
    assert "__launch_bounds__(512)" in sec and "98,688 bytes" in sec
    assert 3 * 32 * 257 * 4 == 98688


def test_wrappers_refuse_cpu_tensors_and_unknown_probes():
    import torch
    from gm3d_amd import knn_probe as KP
    from gm3d_amd import validate as V
    x, y = torch.zeros(16, 8), torch.zeros(16, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        KP.normalize(x)
    with pytest.raises(RuntimeError):
        KP.neighbours(x, x, 3)
    with pytest.raises(RuntimeError):
        KP.knn_classifier(x, y, x, y, 3, 0.07, 2)
    with pytest.raises(ValueError):
        V.validate(None, [], [], probe="nonsense")

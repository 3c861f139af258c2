"""CPU: the linear-SVM entry points (include/gm3d.h, gm3d_amd/csrc/svm.hip) refuse every shape outside their contract on the host,
and the float64 restatement of the solver (tests/svm_ref.py) that the GPU tests trust agrees with sklearn's SVC."""
import ctypes

import numpy as np
import pytest

from tests import svm_ref

ONE = ctypes.c_void_p(16)      # never dereferenced: the shape check fails (or the empty batch returns) first


def _lib():
    from gm3d_amd._capi import lib
    return lib


def _cs(sizes):
    cs = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
    return (ctypes.c_int * len(cs))(*cs), len(sizes), cs[-1]


def _smo(sizes, C=0.01, tol=1e-3):
    arr, ncls, n = _cs(sizes)
    return _lib().gm3d_svm_smo(ONE, n, ncls, arr, C, tol, 0, ONE, ONE, ONE, ONE, None)


def _weights(sizes, d=384):
    arr, ncls, n = _cs(sizes)
    return _lib().gm3d_svm_weights(ONE, n, d, ncls, arr, ONE, ONE, None)


def test_svm_entry_points_refuse_shapes_outside_the_contract():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_OK
    lib = _lib()
    # gram: n <= 16384, d <= 1024
    assert lib.gm3d_svm_gram(ONE, 16385, 384, ONE, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_gram(ONE, 100, 1025, ONE, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_gram(ONE, 0, 384, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_gram(ONE, 100, 0, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_gram(None, 100, 384, ONE, None) == GM3D_EINVAL
    # smo / weights: 2 <= classes <= 64, each pair <= 4096 rows, n <= 16384, consistent class_start
    for call in (_smo, _weights):
        assert call([10]) == GM3D_EUNSUPPORTED                        # one class
        assert call([2] * 65) == GM3D_EUNSUPPORTED                    # 65 classes
        assert call([2049, 2048]) == GM3D_EUNSUPPORTED                # a pair of 4097 rows
        assert call([2049, 2048, 10]) == GM3D_EUNSUPPORTED            # the largest pair is not the first
        assert call([256] * 64 + [1]) == GM3D_EUNSUPPORTED            # 65 classes, n = 16385
        assert call([4096, 4096, 4096, 4097]) == GM3D_EUNSUPPORTED    # n = 16385 beats every other limit
        assert call([5, 0, 5]) == GM3D_EINVAL                         # an empty class
    arr, ncls, n = _cs([3, 3])
    assert lib.gm3d_svm_smo(ONE, n, 0, arr, 0.01, 1e-3, 0, ONE, ONE, ONE, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_smo(ONE, n, ncls, None, 0.01, 1e-3, 0, ONE, ONE, ONE, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_smo(ONE, n + 1, ncls, arr, 0.01, 1e-3, 0, ONE, ONE, ONE, ONE, None) == GM3D_EINVAL   # class_start[ncls] != n
    assert _smo([3, 3], C=0.0) == GM3D_EINVAL
    assert _smo([3, 3], tol=0.0) == GM3D_EINVAL
    assert lib.gm3d_svm_smo(None, n, ncls, arr, 0.01, 1e-3, 0, ONE, ONE, ONE, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_smo(ONE, n, ncls, arr, 0.01, 1e-3, 0, ONE, ONE, ONE, None, None) == GM3D_EINVAL
    assert _weights([3, 3], d=1025) == GM3D_EUNSUPPORTED
    assert _weights([3, 3], d=0) == GM3D_EINVAL
    # predict: classes, d, m <= 16384; m == 0 launches nothing
    assert lib.gm3d_svm_predict(ONE, 10, 384, 1, ONE, ONE, None, ONE, None, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_predict(ONE, 10, 384, 65, ONE, ONE, None, ONE, None, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_predict(ONE, 10, 1025, 40, ONE, ONE, None, ONE, None, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_predict(ONE, 16385, 384, 40, ONE, ONE, None, ONE, None, None) == GM3D_EUNSUPPORTED
    assert lib.gm3d_svm_predict(ONE, -1, 384, 40, ONE, ONE, None, ONE, None, None) == GM3D_EINVAL
    assert lib.gm3d_svm_predict(ONE, 10, 384, 40, ONE, ONE, ONE, ONE, None, None) == GM3D_EINVAL      # labels without a counter
    assert lib.gm3d_svm_predict(ONE, 0, 1024, 64, ONE, ONE, None, ONE, None, None) == GM3D_OK
    assert lib.gm3d_svm_predict(ONE, 0, 1024, 2, ONE, ONE, None, ONE, None, None) == GM3D_OK
    # the last accepted value of each limit passes the checks (run on the GPU in tests/test_gpu_svm.py where it launches)
    # (a NULL data pointer then fails after them with GM3D_EINVAL, so nothing launches)
    for sizes in ([2048, 2048], [4095, 1], [256] * 64, [1, 1]):
        arr, ncls, n = _cs(sizes)
        assert lib.gm3d_svm_smo(None, n, ncls, arr, 0.01, 1e-3, 0, ONE, ONE, ONE, ONE, None) == GM3D_EINVAL
        assert lib.gm3d_svm_weights(None, n, 1024, ncls, arr, ONE, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_gram(None, 16384, 1024, ONE, None) == GM3D_EINVAL
    assert lib.gm3d_svm_predict(None, 16384, 1024, 64, ONE, ONE, None, ONE, None, None) == GM3D_EINVAL


def test_restatement_matches_sklearn():
    pytest.importorskip("sklearn")
    from sklearn.svm import SVC
    for ncls, n, sep, seed in ((6, 600, 1.0, 1), (2, 400, 0.5, 2), (5, 500, 0.6, 3)):
        Xtr, ytr, Xte, yte = svm_ref.synthetic(n, n // 2, ncls, 24, seed=seed, sep=sep)
        ytr, yte = ytr * 7 - 3, yte * 7 - 3                       # non-contiguous labels
        ours = svm_ref.OvO().fit(Xtr, ytr)
        clf = SVC(C=0.01, kernel="linear").fit(Xtr.astype(np.float64), ytr)
        coef, icpt = svm_ref.sklearn_coef(clf)
        assert np.array_equal(ours.classes_, clf.classes_)
        assert np.abs(ours.coef_ - coef).max() <= 1e-2 * np.abs(coef).max()
        assert np.abs(-ours.rho_ - icpt).max() <= 1e-2
        assert np.array_equal(ours.predict(Xte), clf.predict(Xte))
        # the fixed point is a KKT point of every pair
        cs = ours.class_start_
        Xg = Xtr.astype(np.float64)[np.argsort(np.unique(ytr, return_inverse=True)[1], kind="stable")]
        for p, (s, t) in enumerate(svm_ref.pairs(ncls)):
            rows = np.r_[cs[s]:cs[s + 1], cs[t]:cs[t + 1]]
            Kp = Xg[rows] @ Xg[rows].T
            assert svm_ref.kkt_gap(Kp, cs[s + 1] - cs[s], ours.alpha_[p]) < 1e-3 + 1e-9

"""CPU: the linear probe (include/gm3d.h, gm3d_amd/csrc/linprobe.hip, gm3d_amd/linear_probe.py).  The float64 restatement the GPU
tests trust (tests/linear_probe_ref.py) reproduces the committed fixture; its fp32 run sits within half of the parity bar on the inputs
of every GPU case, so the bar tests the kernel and not the number format; the entry points refuse every shape outside their contract on
the host; the header states the limits the wrapper carries."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import linear_probe_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = ctypes.c_void_p(16)      # 16-byte aligned, never dereferenced: a check fails (or the empty range returns) first


def _lib():
    from gm3d_amd._capi import lib
    return lib


def _train(n=100, d=64, ncls=10, batch=20, t0=0, t1=0, momentum=0.9, **ptr):
    names = ("X", "y", "order", "lr", "W", "mom_w", "bias2", "mom_b", "rmean", "rvar", "xhat", "part", "losses")
    p = {k: ptr.get(k, ONE) for k in names}
    return _lib().gm3d_linprobe_train(p["X"], p["y"], n, d, ncls, batch, p["order"], p["lr"], t0, t1, momentum, p["W"], p["mom_w"],
                                      p["bias2"], p["mom_b"], p["rmean"], p["rvar"], p["xhat"], p["part"], p["losses"], None)


def _eval(m=0, d=64, ncls=10, Q=ONE, yq=None, W=ONE, bias=ONE, rmean=ONE, rvar=ONE, correct=None):
    return _lib().gm3d_linprobe_eval(Q, yq, m, d, ncls, W, bias, rmean, rvar, None, None, correct, None)


def test_restatement_reproduces_the_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "linear_probe.npz"))
    f = LR.FIXTURE
    X, y, Qpool, ypool, weight, orders = LR.fixture_inputs()
    # the seeded inputs are the ones the fixture was made from
    assert np.allclose([X.astype(np.float64).sum(), Qpool.astype(np.float64).sum()], z["x_sum"], rtol=1e-9, atol=0)
    assert np.isclose(weight.astype(np.float64).sum(), float(z["w0_sum"]), rtol=1e-9, atol=0)
    assert X.shape == (640, 384) and not X[:, 1].any() and z["rows"].shape == (256,)
    lr = LR.peak_lr(f["batch"])
    # the restated schedule is the reference's, to the bit
    assert np.array_equal(LR.learning_rates(f["epochs"], f["n"] // f["batch"], lr, 0.0, f["warmup_epochs"]), z["rates"])
    from gm3d_amd.linear_probe import learning_rates
    assert np.array_equal(np.asarray(learning_rates(f["epochs"], f["n"] // f["batch"], lr, 0.0, f["warmup_epochs"])).astype(np.float32),
                          z["rates"])
    rows = z["rows"]
    res = LR.fit(X, y, Qpool[rows], ypool[rows], f["num_classes"], weight, orders, f["batch"], f["epochs"], f["warmup_epochs"], lr)
    for k in LR.TENSORS:
        err = LR.rel_err(res[k], z[k])
        print("%s: %.3e" % (k, err))
        assert err <= 1e-9
    assert res["eval_epochs"] == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(np.array(res["hits"]), z["hits"])
    # the stored counts are unambiguous from the second epoch on
    assert (z["min_gap"][1:] > LR.MIN_GAP).all()
    assert all(min(g) > LR.MIN_GAP for g in res["min_gap"][1:])
    # and the fp32 restatement agrees on them
    res32 = LR.fit(X, y, Qpool[rows], ypool[rows], f["num_classes"], weight, orders, f["batch"], f["epochs"], f["warmup_epochs"], lr,
                   dtype=__import__("torch").float32)
    assert res32["hits"][1:] == res["hits"][1:]
    for k in LR.TENSORS:
        assert LR.rel_err(res32[k], z[k]) <= LR.BAR / 2


def test_sampler_orders_are_the_loaders():
    from gm3d_amd.data import epoch_order
    assert LR.default_orders(37, 3, 5) == [epoch_order(37, e, True, 5, 0, 1) for e in range(3)]


@pytest.mark.parametrize("shape", LR.GPU_CASES)
def test_fp32_restatement_sits_within_half_of_the_bar(shape):
    c = LR.case(*shape)
    assert c["Q"].shape[0] == shape[1]
    for k in LR.TENSORS:
        err = LR.rel_err(c["ref32"][k], c["ref"][k])
        print("%s %s: fp32 vs fp64 %.3e" % (shape, k, err))
        assert err <= LR.BAR / 2
    n, _, _, ncls, batch, epochs, _ = shape
    assert len(c["ref"]["losses"]) == epochs * (n // batch)
    # the margin rule holds where select_rows applied it: those epochs' counts depend on no rounding
    for e, gap, h, h32 in zip(c["ref"]["eval_epochs"], c["ref"]["min_gap"], c["ref"]["hits"], c["ref32"]["hits"]):
        if e >= min(2, epochs):
            assert min(gap) > LR.MIN_GAP and h == h32


def test_entry_points_refuse_shapes_outside_the_contract():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_OK
    lib = _lib()
    assert lib.gm3d_linprobe_slices(384) == 24 and lib.gm3d_linprobe_slices(8) == 1 and lib.gm3d_linprobe_slices(72) == 5
    assert lib.gm3d_linprobe_slices(0) == 0
    # t_begin == t_end launches nothing: every accepted limit returns OK, every refused one its code
    assert _train() == GM3D_OK
    assert _train(n=16384, d=1024, ncls=64, batch=1024) == GM3D_OK
    assert _train(n=2, d=8, ncls=2, batch=2) == GM3D_OK
    assert _train(n=0) == GM3D_EINVAL
    assert _train(n=16385) == GM3D_EUNSUPPORTED
    assert _train(d=0) == GM3D_EINVAL
    assert _train(d=4) == GM3D_EUNSUPPORTED
    assert _train(d=100) == GM3D_EUNSUPPORTED
    assert _train(d=1032) == GM3D_EUNSUPPORTED
    assert _train(ncls=0) == GM3D_EINVAL
    assert _train(ncls=1) == GM3D_EUNSUPPORTED
    assert _train(ncls=65) == GM3D_EUNSUPPORTED
    assert _train(batch=1) == GM3D_EINVAL
    assert _train(batch=101) == GM3D_EINVAL                            # above n
    assert _train(n=2000, batch=1025) == GM3D_EUNSUPPORTED
    assert _train(t0=-1) == GM3D_EINVAL
    assert _train(t0=3, t1=2) == GM3D_EINVAL
    for bad in (-0.1, 1.0, float("nan")):
        assert _train(momentum=bad) == GM3D_EINVAL
    # with iterations to run, the pointer checks still come before any launch
    for name in ("X", "y", "order", "lr", "W", "mom_w", "bias2", "mom_b", "rmean", "rvar", "xhat", "part", "losses"):
        assert _train(t1=1, **{name: None}) == GM3D_EINVAL, name
    assert _train(t1=1, X=ctypes.c_void_p(20)) == GM3D_EINVAL          # not 16-byte aligned
    assert _train(t1=1, xhat=ctypes.c_void_p(24)) == GM3D_EINVAL
    assert _train(t1=1, d=100) == GM3D_EUNSUPPORTED
    # evaluation: m == 0 launches nothing, after the shape checks
    assert _eval() == GM3D_OK
    assert _eval(d=1024, ncls=64) == GM3D_OK and _eval(d=8, ncls=2) == GM3D_OK
    assert _eval(m=-1) == GM3D_EINVAL
    assert _eval(d=0) == GM3D_EINVAL
    assert _eval(d=12) == GM3D_EUNSUPPORTED
    assert _eval(d=1032) == GM3D_EUNSUPPORTED
    assert _eval(ncls=0) == GM3D_EINVAL
    assert _eval(ncls=1) == GM3D_EUNSUPPORTED
    assert _eval(ncls=65) == GM3D_EUNSUPPORTED
    for name in ("Q", "W", "bias", "rmean", "rvar"):
        assert _eval(m=5, **{name: None}) == GM3D_EINVAL, name
    assert _eval(m=5, yq=ONE, correct=None) == GM3D_EINVAL             # labels without counters
    assert _eval(m=5, d=100) == GM3D_EUNSUPPORTED


def test_header_states_the_limits_of_the_wrapper():
    from gm3d_amd import linear_probe as LP
    txt = open(os.path.join(ROOT, "include", "gm3d.h")).read()
    sec = txt[txt.index("Linear probe of pretrained features"):]
    sec = sec[:sec.index("int gm3d_linprobe_slices")]
    line = re.search(r"1 <= n <= (\d+), m >= 0, (\d+) <= d <= (\d+), d % (\d+) == 0, 2 <= ncls <= (\d+), 2 <= batch <= min\(n, (\d+)\)", sec)
    assert line, "the limits line of the linear probe section"
    assert tuple(int(v) for v in line.groups()) == (LP.MAX_N, LP.MIN_D, LP.MAX_D, LP.D_MULTIPLE, LP.MAX_CLASSES, LP.MAX_BATCH)
    src = open(os.path.join(ROOT, "gm3d_amd", "csrc", "linprobe.hip")).read()
    consts = re.search(r"LP_MAX_N = (\d+), LP_MAX_D = (\d+), LP_MAX_CLS = (\d+), LP_MAX_BATCH = (\d+);", src)
    assert tuple(int(v) for v in consts.groups()) == (LP.MAX_N, LP.MAX_D, LP.MAX_CLASSES, LP.MAX_BATCH)
    assert "__launch_bounds__(512)" in sec and "94,720 bytes" in sec and "LP_LDS == 94720" in src
    assert (64 * 16 + 8 * 64 + 32 * 16 + 64 + 64 * 257 + 256 * 20) * 4 == 94720


def test_wrappers_refuse_cpu_tensors_and_unknown_probes():
    import torch
    from gm3d_amd import linear_probe as LP
    from gm3d_amd import validate as V
    x, y = torch.zeros(16, 8), torch.zeros(16, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        LP.LinearProbe(2, batch_size=4).fit(x, y)
    with pytest.raises(RuntimeError):
        LP.linear_probe(x, y, x, y, 2, batch_size=4, epochs=1)
    probe = LP.LinearProbe(2, batch_size=4)
    with pytest.raises(RuntimeError):
        probe.predict(x)                                               # not fitted
    probe.weight = x[:2]
    with pytest.raises(RuntimeError):
        probe.predict(x)
    with pytest.raises(RuntimeError):
        probe.score(x, y)
    with pytest.raises(ValueError):
        LP.LinearProbe(1)
    with pytest.raises(ValueError):
        LP.LinearProbe(10, batch_size=1)
    with pytest.raises(ValueError):
        V.validate(None, [], [], probe="nonsense")

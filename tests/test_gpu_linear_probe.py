"""GPU: the linear probe (gm3d_amd/csrc/linprobe.hip, gm3d_amd/linear_probe.py) against its float64 restatement
(tests/linear_probe_ref.py) and the committed fixture (tests/golden/linear_probe.npz); validate(probe="linear" / "all") end to end.
The bar is the project's parity bar, 1e-5 of max |reference| per tensor; the fp32 restatement sits within half of it on the same
inputs (tests/test_linear_probe_cpu.py).  Hit counts are compared for equality wherever the float64 logits keep a gap above 1e-3 at
ranks 1|2 and 5|6."""
import os

import numpy as np
import pytest
import torch

from tests import linear_probe_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fit(c, num_classes, batch, epochs, weight=True, orders=True, test=True, **kw):
    from gm3d_amd import linear_probe as LP
    probe = LP.LinearProbe(num_classes, batch_size=batch, epochs=epochs, warmup_epochs=c["warmup_epochs"], lr=c["lr"], **kw)
    return probe.fit(_cuda(c["X"]), _cuda(c["y"]), _cuda(c["Q"]) if test else None, _cuda(c["yq"]) if test else None,
                     weight=_cuda(c["weight"]) if weight else None, orders=c["orders"] if orders else None)


def _outputs(probe):
    return [probe.weight, probe.bias, probe.running_mean, probe.running_var, probe.losses]


def _check(probe, ref, name, total):
    for k, got in zip(LR.TENSORS, _outputs(probe)):
        got = got.cpu().numpy()
        assert got.shape == ref[k].shape and np.isfinite(got).all(), (name, k)
        err = LR.rel_err(got, ref[k])
        print("%s %s: %.3e of the bar" % (name, k, err / LR.BAR))
        assert err <= LR.BAR, (name, k, err)
    assert probe.eval_epochs == ref["eval_epochs"]
    compared = 0
    for e, gap, want, got in zip(ref["eval_epochs"], ref["min_gap"], ref["hits"], probe.history):
        hits = (round(got[0] * total / 100.0), round(got[1] * total / 100.0))
        print("%s epoch %d: hits %s, float64 %s, smallest gap %.2e" % (name, e, hits, want, min(gap)))
        if min(gap) > LR.MIN_GAP:
            assert hits == tuple(want), (name, e)
            compared += 1
    return compared


@pytest.mark.parametrize("shape", LR.GPU_CASES)
def test_fit_matches_float64(shape):
    n, m, d, ncls, batch, epochs, offset = shape
    c = LR.case(*shape)
    probe = _fit(c, ncls, batch, epochs)
    assert _check(probe, c["ref"], str(shape), m) >= max(epochs - 1, 1)
    if ncls == 2:
        assert all(h[1] == 100.0 for h in probe.history)            # top-5 = top-min(5, C): both classes
    # predict / score are the evaluation of the last epoch
    assert round(probe.score(_cuda(c["Q"]), _cuda(c["yq"])) * m) == round(probe.history[-1][0] * m / 100.0)
    pred = probe.predict(_cuda(c["Q"]))
    assert int((pred.cpu().numpy() == c["yq"]).sum()) == round(probe.history[-1][0] * m / 100.0)


def test_fit_reproduces_the_committed_fixture():
    """The seed path: the initial weights and the orders are drawn by LinearProbe itself."""
    from gm3d_amd import linear_probe as LP
    z = np.load(os.path.join(ROOT, "tests", "golden", "linear_probe.npz"))
    f = LR.FIXTURE
    X, y, Qpool, ypool, _, _ = LR.fixture_inputs()
    Q, yq = Qpool[z["rows"]], ypool[z["rows"]]
    res = LP.linear_probe(_cuda(X), _cuda(y), _cuda(Q), _cuda(yq), f["num_classes"], batch_size=f["batch"], epochs=f["epochs"],
                          warmup_epochs=f["warmup_epochs"], seed=f["seed"])      # blr 0.1: lr = 0.1 * batch / 256
    probe = LP.LinearProbe(f["num_classes"], batch_size=f["batch"], epochs=f["epochs"], warmup_epochs=f["warmup_epochs"], seed=f["seed"])
    probe.fit(_cuda(X), _cuda(y), _cuda(Q), _cuda(yq))
    ref = {k: z[k] for k in LR.TENSORS}
    ref.update(eval_epochs=list(range(1, f["epochs"] + 1)), min_gap=z["min_gap"].tolist(), hits=z["hits"].tolist())
    assert _check(probe, ref, "fixture", f["m"]) >= f["epochs"] - 1
    assert res["history"] == probe.history
    assert (res["acc1"], res["acc5"]) == probe.history[-1] and res["max_acc1"] == max(h[0] for h in probe.history)
    assert res["acc1"] == z["hits"][-1][0] * 100.0 / f["m"] and res["acc5"] == z["hits"][-1][1] * 100.0 / f["m"]


SMALL = (96, 40, 24, 5, 32, 4, 3.0)      # n, m, d, C, batch, epochs, offset


def test_batch_of_all_rows_is_one_iteration_per_epoch():
    n, m, d, ncls, _, epochs, _ = SMALL
    c = LR.case(*SMALL)
    ref = LR.fit(c["X"], c["y"], c["Q"], c["yq"], ncls, c["weight"], c["orders"], n, epochs, 1, c["lr"])
    probe = _fit(c, ncls, n, epochs)
    assert probe.losses.numel() == epochs
    _check(probe, ref, "batch == n", m)


def test_eval_every_second_epoch_and_the_last():
    n, m, d, ncls, batch, _, _ = SMALL
    c = LR.case(*SMALL[:5], 5)
    ref = LR.fit(c["X"], c["y"], c["Q"], c["yq"], ncls, c["weight"], c["orders"], batch, 5, 1, c["lr"], eval_every=2)
    assert ref["eval_epochs"] == [2, 4, 5]
    probe = _fit(c, ncls, batch, 5, eval_every=2)
    assert len(probe.history) == 3
    _check(probe, ref, "eval_every=2", m)
    # the training does not depend on when it is evaluated
    every = _fit(c, ncls, batch, 5)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(probe), _outputs(every)))
    assert [every.history[i] for i in (1, 3, 4)] == probe.history


def test_no_test_rows():
    from gm3d_amd import linear_probe as LP
    n, m, d, ncls, batch, epochs, _ = SMALL
    c = LR.case(*SMALL)
    full = _fit(c, ncls, batch, epochs)
    none = _fit(c, ncls, batch, epochs, test=False)
    assert none.history == [] and none.eval_epochs == []
    empty = dict(c, Q=c["Q"][:0], yq=c["yq"][:0])
    zero = _fit(empty, ncls, batch, epochs)
    assert zero.history == [(0.0, 0.0)] * epochs
    for p in (none, zero):
        assert all(torch.equal(a, b) for a, b in zip(_outputs(p), _outputs(full)))
    assert full.predict(_cuda(empty["Q"])).shape == (0,)
    with pytest.raises(ValueError):
        LP.LinearProbe(ncls, batch_size=batch, epochs=1).fit(_cuda(c["X"]), _cuda(c["y"]).clamp(max=ncls - 1) + 1)      # label C
    with pytest.raises(ValueError):
        LP.LinearProbe(ncls, batch_size=n + 1, epochs=1).fit(_cuda(c["X"]), _cuda(c["y"]))


def test_injected_orders_with_a_repeated_row():
    n, m, d, ncls, batch, epochs, _ = SMALL
    c = LR.case(*SMALL)
    orders = [list(o) for o in c["orders"]]
    for o in orders:
        o[1] = o[0]                                                 # the same row twice in the first batch
        o[batch + 3] = o[2]                                         # and one row in two batches
    ref = LR.fit(c["X"], c["y"], c["Q"], c["yq"], ncls, c["weight"], orders, batch, epochs, 1, c["lr"])
    probe = _fit(dict(c, orders=orders), ncls, batch, epochs)
    _check(probe, ref, "repeated rows", m)
    plain = _fit(c, ncls, batch, epochs)
    assert not torch.equal(plain.weight, probe.weight)
    with pytest.raises(ValueError):
        _fit(dict(c, orders=[o[:-1] + [n] for o in orders]), ncls, batch, epochs)


def test_two_fits_are_equal_bit_for_bit():
    shape = LR.GPU_CASES[3]
    n, m, d, ncls, batch, epochs, _ = shape
    c = LR.case(*shape)
    a, b = _fit(c, ncls, batch, epochs), _fit(c, ncls, batch, epochs)
    assert all(torch.equal(u, v) for u, v in zip(_outputs(a), _outputs(b)))
    assert a.history == b.history
    assert torch.equal(a.predict(_cuda(c["Q"])), b.predict(_cuda(c["Q"])))


@pytest.mark.parametrize("pattern", ["nan", "+inf", "-inf"])
def test_no_result_depends_on_unwritten_memory(pattern):
    """Every allocation of gm3d_amd/linear_probe.py filled with NaN / +inf / -inf (tests/poison.py) before a kernel writes it: the fit,
    the predictions and evaluate_linear's dict are the same bits as without.  The sites stay recorded in poison.SITES: they count as
    reached for the coverage condition of the poison modules, which run after this one."""
    from gm3d_amd import validate as V
    from tests import poison
    n, m, d, ncls, batch, epochs, _ = SMALL
    c = LR.case(*SMALL)

    def run():
        probe = _fit(c, ncls, batch, epochs, weight=False)          # the seed path draws into an empty host tensor
        res = V.evaluate_linear(_cuda(c["X"]).view(n, 1, d).expand(n, 2, d) * 0.5, _cuda(c["y"]), _cuda(c["Q"]), _cuda(c["yq"]),
                                batch_size=batch, epochs=2, warmup_epochs=1)
        return [t.cpu() for t in _outputs(probe)] + [probe.predict(_cuda(c["Q"])).cpu()], (probe.history, res)

    want, want_acc = run()
    with poison.poisoned(pattern) as ps:
        got, got_acc = run()
    sites = poison.scan_sites()
    mine = {s for s in sites if s.startswith("gm3d_amd/linear_probe.py:")}
    assert mine and mine <= ps.sites, sorted(mine - ps.sites)
    assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(want, got))
    assert want_acc == got_acc
    assert all(np.isfinite(a.numpy()).all() for a in want)


# ---- validate(probe=) end to end ---------------------------------------------------------------------------------------------------

def _loader(n, ncls, batch, seed):
    """(taxonomy_ids, model_ids, (points (B,8192,3), label (B,))) batches: class c is an ellipsoid with its own axes."""
    g = torch.Generator().manual_seed(seed)
    axes = torch.tensor([[1.0, 0.3 + 0.2 * c, 0.5] for c in range(ncls)])
    out = []
    for b0 in range(0, n, batch):
        bs = min(batch, n - b0)
        lab = torch.arange(b0, b0 + bs) % ncls
        d = torch.randn(bs, 8192, 3, generator=g)
        pts = d / d.norm(dim=-1, keepdim=True) * axes[lab][:, None, :]
        pts = pts + 0.02 * torch.randn(bs, 8192, 3, generator=g)
        out.append((None, None, (pts, lab)))
    return out


def _validate_probes(model, npoints):
    from gm3d_amd import validate as V
    train, test = _loader(8, 2, 4, seed=1), _loader(4, 2, 4, seed=2)      # batches of B = 4 clouds
    kw = {"epochs": 3, "warmup_epochs": 1, "batch_size": 4}
    linear = V.validate(model, train, test, npoints=npoints, probe="linear", linear_kwargs=kw)
    acc, knn, lin2 = V.validate(model, train, test, npoints=npoints, svm_backend="hip", probe="all", knn_ks=(2, 4), linear_kwargs=kw)
    both = V.validate(model, train, test, npoints=npoints, svm_backend="hip", probe="both", knn_ks=(2, 4))
    assert isinstance(both, tuple) and len(both) == 2 and both == (acc, knn)
    assert lin2 == linear
    feats, was_training = [], model.training
    model.eval()                                                    # as validate() extracts
    for loader in (train, test):
        f = torch.cat([V.pool_features(V.extract_features(model, d[0].cuda(), npoints)) for _, _, d in loader], 0)
        feats += [f, torch.cat([d[1] for _, _, d in loader], 0).cuda()]
    model.train(was_training)
    assert linear == V.evaluate_linear(*feats, **kw)
    assert set(linear) == {"acc1", "acc5", "max_acc1", "history"} and len(linear["history"]) == 3
    assert 0.0 <= linear["acc1"] <= linear["max_acc1"] <= 100.0 and linear["acc5"] == 100.0      # two classes
    # a default batch above the training rows is lowered to them
    assert V.evaluate_linear(*feats, epochs=3, warmup_epochs=1) == V.evaluate_linear(*feats, epochs=3, warmup_epochs=1, batch_size=8)


def test_validate_probe_point_mae():
    from gm3d_amd import models_mae_learn_loss as M
    from oracle import model_ref as R
    torch.manual_seed(0)
    m = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(), seed=0).cuda().train()
    _validate_probes(m, None)
    assert m.training


def test_validate_probe_point_m2ae():
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    _validate_probes(P.PointM2AE().cuda().eval(), 2048)

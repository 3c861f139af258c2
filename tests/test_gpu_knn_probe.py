"""GPU: the weighted k-NN probe (gm3d_amd/csrc/knn_probe.hip, gm3d_amd/knn_probe.py) against its float64 restatement
(tests/knn_probe_ref.py) and the reference's own results (tests/golden/knn_probe.npz); validate(probe=) end to end."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import knn_probe_ref as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.07
MIN_GAP, MIN_MARGIN, MAX_EXCLUDED = 1e-4, 1e-3, 0.05


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- lattice inputs: every dot product is exact in any order, so idx and sim are equalities -------------------------------------

def _lattice(n, m, d, seed):
    r = np.random.RandomState(seed)
    return (r.randint(-1, 2, (n, d)) * 0.125).astype(np.float32), (r.randint(-1, 2, (m, d)) * 0.125).astype(np.float32)


@pytest.mark.parametrize("n,m,d,k", [(1027, 37, 64, 20), (257, 33, 8, 256), (5, 3, 1024, 5), (300, 1, 64, 1)])
def test_neighbours_exact_on_lattice_inputs(n, m, d, k):
    from gm3d_amd import knn_probe as KP
    X, Q = _lattice(n, m, d, seed=n + k)
    idx, sim = KP.neighbours(_cuda(X), _cuda(Q), k)
    ridx, rsim, _ = KR.neighbours(X, Q, k)
    if n > 100 and k > 1:
        assert (np.diff(rsim, axis=1) == 0).any()                  # the lattice is full of ties: the index rule decides
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.array_equal(sim.cpu().numpy(), rsim.astype(np.float32))


def test_neighbours_of_an_all_equal_input_are_the_first_rows():
    from gm3d_amd import knn_probe as KP
    X = np.full((700, 64), 0.125, np.float32)
    idx, sim = KP.neighbours(_cuda(X), _cuda(X[:40]), 37)
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(37), (40, 1)))
    assert np.array_equal(sim.cpu().numpy(), np.full((40, 37), 1.0, np.float32))


def test_classify_ranks_equal_and_unvoted_classes_by_id():
    from gm3d_amd import knn_probe as KP
    X = np.full((7, 8), 0.125, np.float32)
    lab = torch.tensor([3, 3, 1, 1, 0, 0, 0]).cuda()
    top5, probs, correct = KP.classify(_cuda(X), lab, _cuda(X[:2]), 4, T, 5, test_labels=torch.tensor([1, 0]).cuda(), return_probs=True)
    assert top5.tolist() == [[1, 3, 0, 2, 4]] * 2
    assert correct.tolist() == [1, 2]                               # label 0 is the third of min(5, k, ncls) = 4 ranks
    w = np.exp(np.float32(0.125) / np.float32(T))
    assert np.allclose(probs.cpu().numpy(), [[0, 2 * w, 0, 2 * w, 0]] * 2, rtol=1e-6)
    top5, _, _ = KP.classify(_cuda(X), lab.clamp(max=1), _cuda(X[:2]), 4, T, 2)
    assert top5.tolist() == [[1, 0, -1, -1, -1]] * 2                # two classes: rows 0..3 all vote for class 1, -1 beyond ncls


# ---- the reference's own fixture -----------------------------------------------------------------------------------------------

def test_knn_classifier_reproduces_the_reference_fixture():
    from gm3d_amd import knn_probe as KP
    z = np.load(os.path.join(ROOT, "tests", "golden", "knn_probe.npz"))
    xtr, xte = _cuda(z["train"]), _cuda(z["test"])
    ytr, yte = _cuda(z["train_labels"].astype(np.int64)), _cuda(z["test_labels"].astype(np.int64))
    for k, (top1, top5) in zip(z["ks"].tolist(), z["top"].tolist()):
        assert KP.knn_classifier(xtr, ytr, xte, yte, k, float(z["T"]), int(z["num_classes"])) == (top1, top5)
    assert KP.knn_classifier(xtr, ytr, xte, yte, 10, float(z["T"])) == tuple(z["top"][0].tolist())    # num_classes from the labels
    with pytest.raises(ValueError):
        KP.knn_classifier(xtr, ytr, xte, yte, 10, float(z["T"]), 9)                                  # label 9 outside 0..8


# ---- clustered Gaussian features ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clustered(d, ncls, seed=0, n=2000, m=300, groups=10):
    """Ten groups of 200 training rows (group centre 3, class offset 1.5, noise of a per-row scale in 1.6 .. 6.4, then L2-normalised):
    the similarities of a test row spread widely inside its group and fall off behind it, so the k | k+1 boundary of few rows is
    closer than 1e-4.  Seed 0 was chosen with the restatement alone: it excludes at most 3.3 % of the rows of any case below."""
    r = np.random.RandomState(seed)
    C, D = r.randn(groups, d) / np.sqrt(d), r.randn(ncls, d) / np.sqrt(d)

    def rows(cnt):
        i = np.arange(cnt)
        s = 4.0 * r.uniform(0.4, 1.6, (cnt, 1))
        x = 3.0 * C[i % groups] + 1.5 * D[i % ncls] + s * r.randn(cnt, d) / np.sqrt(d)
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        return x.astype(np.float32), (i % ncls).astype(np.int64)
    return rows(n) + rows(m)


@functools.lru_cache(maxsize=None)
def _clustered_ref(d, ncls, k):
    xtr, ytr, xte, yte = _clustered(d, ncls)
    return KR.knn_classifier(xtr, ytr, xte, yte, k, T, ncls)


@pytest.mark.parametrize("k", [10, 200])
@pytest.mark.parametrize("ncls", [40, 15])
@pytest.mark.parametrize("d", [384, 768])
def test_classify_matches_float64_on_clustered_features(d, ncls, k):
    from gm3d_amd import knn_probe as KP
    xtr, ytr, xte, yte = _clustered(d, ncls)
    ref = _clustered_ref(d, ncls, k)
    top5, probs, correct = KP.classify(_cuda(xtr), _cuda(ytr), _cuda(xte), k, T, ncls, test_labels=_cuda(yte), return_probs=True)
    top5, probs = top5.cpu().numpy(), probs.cpu().numpy().astype(np.float64)
    sure = (ref["gap"] > MIN_GAP) & (ref["margin12"] > MIN_MARGIN) & (ref["margin56"] > MIN_MARGIN)
    excluded = 1.0 - sure.mean()
    print("d %d ncls %d k %d: excluded %.4f" % (d, ncls, k, excluded))
    assert excluded <= MAX_EXCLUDED
    # the scores, where the neighbour set is decided (the boundary gap is far above fp32's 1e-7)
    rows = ref["gap"] > MIN_GAP
    rel = np.abs(probs[rows] - ref["probs"][rows]) / np.where(ref["probs"][rows] > 0, ref["probs"][rows], 1.0)
    print("probs: max relative error %.3e" % rel.max())
    assert np.array_equal(probs[rows] == 0, ref["probs"][rows] == 0)
    assert rel.max() <= 1e-5
    # predictions and top-5 membership on every unambiguous row
    assert np.array_equal(top5[sure, 0], ref["ranking"][sure, 0])
    assert np.array_equal(np.sort(top5[sure], 1), np.sort(ref["ranking"][sure, :5], 1))
    if excluded == 0.0:
        m = xte.shape[0]
        assert correct.tolist() == [round(ref["top1"] * m / 100.0), round(ref["top5"] * m / 100.0)]


# ---- normalize -------------------------------------------------------------------------------------------------------------------

def test_normalize_matches_torch():
    from gm3d_amd import knn_probe as KP
    g = torch.Generator().manual_seed(3)
    for n, d in ((37, 384), (5, 8), (9, 1000)):
        x = torch.randn(n, d, generator=g) * 3.0
        x[1] = 0.0                                                  # an all-zero row stays zero
        x[2] = 0.0
        x[2, 0] = 1e-20                                             # norm 1e-20 < eps: divided by 1e-12
        want = torch.nn.functional.normalize(x, p=2, dim=1)
        got = KP.normalize(x.cuda()).cpu()
        assert torch.isfinite(got).all()
        assert (got - want).abs().max().item() <= 1e-6
        assert torch.equal(got[1], torch.zeros(d))
        assert got[2, 0].item() == pytest.approx(1e-8, rel=1e-6)


# ---- reproducibility and counters ----------------------------------------------------------------------------------------------------

def test_outputs_are_reproducible_and_counters_accumulate():
    from gm3d_amd import knn_probe as KP
    xtr, ytr, xte, yte = (_cuda(a) for a in _clustered(384, 40))
    a = KP.neighbours(xtr, xte, 100) + KP.classify(xtr, ytr, xte, 100, T, 40, test_labels=yte, return_probs=True)
    b = KP.neighbours(xtr, xte, 100) + KP.classify(xtr, ytr, xte, 100, T, 40, test_labels=yte, return_probs=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    once = a[4].clone()
    assert once[0] > 0 and once[1] >= once[0]
    KP.classify(xtr, ytr, xte, 100, T, 40, test_labels=yte, correct=a[4])
    assert torch.equal(a[4], 2 * once)                              # +=
    # without test labels nothing is counted (and no counter is needed)
    top5, _, correct = KP.classify(xtr, ytr, xte, 100, T, 40)
    assert correct is None and torch.equal(top5, a[2])
    from gm3d_amd import _capi
    from gm3d_amd.ops import _ptr, _stream
    sentinel = torch.tensor([-7, 11], dtype=torch.int64).cuda()
    n, d = xtr.shape
    _capi.check(_capi.lib.gm3d_knn_probe_classify(_ptr(xtr), _ptr(xte), n, xte.shape[0], d, 100, _ptr(ytr), 40, T, None, _ptr(top5), None,
                                                  _ptr(sentinel), _stream()), "gm3d_knn_probe_classify")
    assert sentinel.tolist() == [-7, 11]


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
    train, test = _loader(40, 4, 20, seed=1), _loader(24, 4, 12, seed=2)
    ks = (10, 20, 40)                                              # the reference's ks clipped to the 40 training clouds
    svm = V.validate(model, train, test, npoints=npoints, svm_backend="hip")
    acc, knn = V.validate(model, train, test, npoints=npoints, svm_backend="hip", probe="both", knn_ks=ks)
    assert acc == svm
    assert V.validate(model, train, test, npoints=npoints, probe="knn", knn_ks=ks) == knn
    feats, was_training = [], model.training
    model.eval()                                                    # as validate() extracts
    for loader in (train, test):
        f = torch.cat([V.pool_features(V.extract_features(model, d[0].cuda(), npoints)) for _, _, d in loader], 0)
        feats += [f, torch.cat([d[1] for _, _, d in loader], 0).cuda()]
    model.train(was_training)
    assert knn == V.evaluate_knn(*feats, ks=ks)
    assert set(knn) == set(ks)
    for top1, top5 in knn.values():
        assert 0.0 <= top1 <= top5 <= 100.0
    assert knn[40][1] == 100.0                                      # four classes: the label is always among the first four
    with pytest.warns(UserWarning, match="skipped"):
        assert set(V.evaluate_knn(*feats, ks=(10, 100))) == {10}    # k above the training rows is skipped, and said so


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

"""-m gpu: device-resident datasets (gm3d_amd/data.py, gm3d_amd/csrc/dataset.hip) -- gm3d_sample_normalize against the reference's
own random_sample + pc_norm (tests/golden/shapenet_dataset.npz, made by tests/golden/make_golden_dataset.py) and against a NumPy
restatement, its tie rules, the loader's determinism, labels and rank split, and the loader plugged into the Point-MAE engine."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -24          # fp32 unit roundoff


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "shapenet_dataset.npz"))


def _run(data, cloud_idx, keys, num, normalize):
    from gm3d_amd import data as D
    out, idx = D.sample_normalize(torch.from_numpy(data).cuda(), torch.from_numpy(np.asarray(cloud_idx, dtype=np.int64)).cuda(),
                                  torch.from_numpy(keys).cuda(), num, normalize, return_idx=True)
    return out.cpu().numpy(), idx.cpu().numpy()


# --------------------------------------------------------------------------- against the reference's fixture
@pytest.mark.parametrize("case", ["n2048_256", "n8192_1024", "n33_7"])
def test_against_the_reference_fixture(fx, case):
    """Keys built from the permutation the reference drew (keys[perm[j]] = j / N0, exact in fp32 order) select its points in its
    order; the normalised output stays within max(the reference's own fp32 error against float64, 8 * 2^-24) of the float64
    pc_norm.  The bar is applied per cloud, which is no looser than per case."""
    clouds, perm, num = fx[case + "/clouds"], fx[case + "/perm"].astype(np.int64), int(fx[case + "/num"])
    M, N0, _ = clouds.shape
    keys = np.empty((M, N0), dtype=np.float32)
    for b in range(M):
        keys[b, perm[b]] = np.arange(N0, dtype=np.float32) / np.float32(N0)
    out, idx = _run(clouds, np.arange(M), keys, num, 1)
    assert np.array_equal(idx, perm[:, :num])
    raw, idx0 = _run(clouds, np.arange(M), keys, num, 0)
    assert np.array_equal(idx0, idx)
    assert all(np.array_equal(raw[b], clouds[b][perm[b, :num]]) for b in range(M))
    err = np.abs(out.astype(np.float64) - fx[case + "/out64"]).reshape(M, -1).max(1)
    ref_err = fx[case + "/ref_err"]
    for b in range(M):
        print("%s cloud %d: error vs float64 %.3e, the reference's own %.3e" % (case, b, err[b], ref_err[b]))
    assert err.max() <= max(ref_err.max(), 8 * U)                       # the bar as stated, per case
    assert all(err[b] <= max(ref_err[b], 8 * U) for b in range(M))     # and per cloud


# --------------------------------------------------------------------------- against a NumPy restatement
def _restate(data, cloud_idx, keys, num, normalize):
    idx = np.argsort(keys, axis=1, kind="stable")[:, :num]
    pts = np.stack([data[c][i] for c, i in zip(cloud_idx, idx)])
    if not normalize:
        return pts, idx
    p = pts.astype(np.float64)
    p = p - p.mean(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p / np.sqrt((p ** 2).sum(-1)).max(1)[:, None, None], idx


def _tolerance(pts, out64):
    """fp32 error bound of the kernel's pc_norm for coordinates |x| <= a and scale m (both from the inputs and the float64
    restatement, not from the kernel): the longest chain of additions into a coordinate sum is 7 (a thread's rows) + 6 (the wave
    butterfly) + 15 (the wave sums) = 28, so |sum error| / num <= 28 u a; the division by num adds u a and the subtraction u |c|
    with |c| <= 2a: at most 31 u a / m after the division by the scale.  The scale (three products, two sums, one square root) is
    off by under 3 u relatively and the last division by u, on outputs of magnitude <= 1: 4 u more."""
    a = np.abs(pts).max()
    c = pts.astype(np.float64)
    c = c - c.mean(1, keepdims=True)
    m = np.sqrt((c ** 2).sum(-1)).max(1).min()
    return U * (31.0 * a / m + 4.0)


SHAPES = [(N0, num, B) for N0 in (1, 33, 64, 2048, 8192) for num in sorted({1, N0 - 1, N0}) if num >= 1 for B in (1, 3)]


@pytest.mark.parametrize("N0,num,B", SHAPES)
def test_against_numpy_restatement(N0, num, B):
    rng = np.random.RandomState(1000 * N0 + 10 * num + B)
    M = 4
    data = rng.uniform(-1, 1, (M, N0, 3)).astype(np.float32)
    cloud_idx = [3, 1, 1][:B]                                  # descending, with a repeat
    keys = rng.uniform(0, 1, (B, N0)).astype(np.float32)
    want, widx = _restate(data, cloud_idx, keys, num, False)
    got, idx = _run(data, cloud_idx, keys, num, 0)
    assert np.array_equal(idx, widx)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want))          # bit copies
    want64, _ = _restate(data, cloud_idx, keys, num, True)
    out, idx1 = _run(data, cloud_idx, keys, num, 1)
    assert np.array_equal(idx1, widx)
    if num == 1:                                               # one point: 0 / 0, as in the reference
        assert np.isnan(out).all() and np.isnan(want64).all()
        return
    tol = _tolerance(want, want64)
    err = np.abs(out.astype(np.float64) - want64).max()
    print("N0 %d num %d B %d: error %.3e, bound %.3e" % (N0, num, B, err, tol))
    assert err <= tol


# --------------------------------------------------------------------------- ties and odd keys
def _odd_keys(kind, B, N0, rng):
    if kind == "four_values":
        return (rng.randint(0, 4, (B, N0)) / 4.0).astype(np.float32)
    if kind == "all_equal":
        return np.full((B, N0), 0.5, dtype=np.float32)
    if kind == "signed_zeros":
        return np.where(rng.randint(0, 2, (B, N0)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    keys = rng.uniform(0, 1, (B, N0)).astype(np.float32)     # two NaNs per row
    keys[:, 5] = np.nan
    keys[:, N0 // 2] = np.nan
    return keys


@pytest.mark.parametrize("kind", ["four_values", "all_equal", "signed_zeros", "two_nans"])
@pytest.mark.parametrize("N0,num", [(33, 20), (300, 300), (2048, 2047)])
def test_ties_and_odd_keys(kind, N0, num):
    rng = np.random.RandomState(N0 + len(kind))
    B, M = 3, 3
    data = rng.uniform(-1, 1, (M, N0, 3)).astype(np.float32)
    keys = _odd_keys(kind, B, N0, rng)
    cloud_idx = [2, 0, 2]
    out, idx = _run(data, cloud_idx, keys, num, 1)
    full, fidx = _run(data, cloud_idx, keys, N0, 0)
    for b in range(B):
        assert idx[b].min() >= 0 and idx[b].max() < N0 and len(set(idx[b].tolist())) == num
        assert sorted(fidx[b].tolist()) == list(range(N0))
    _, widx = _restate(data, cloud_idx, keys, N0, False)     # stable argsort: equal keys (and -0 / +0) by index, NaN last
    assert np.array_equal(fidx, widx) and np.array_equal(idx, widx[:, :num])
    if kind in ("all_equal", "signed_zeros"):
        assert np.array_equal(fidx, np.tile(np.arange(N0), (B, 1)))
        assert all(np.array_equal(full[b], data[cloud_idx[b]]) for b in range(B))
    if kind == "two_nans":
        assert np.array_equal(fidx[:, -2:], np.tile([5, N0 // 2], (B, 1)))
    out2, idx2 = _run(data, cloud_idx, keys, num, 1)          # a second call: bit-identical
    assert np.array_equal(idx2, idx) and out2.tobytes() == out.tobytes()


# --------------------------------------------------------------------------- the loader
def _dataset(M=10, N0=64, labels=False, **kw):
    from gm3d_amd import data as D
    pts = np.random.RandomState(5).uniform(-1, 1, (M, N0, 3)).astype(np.float32)
    return D.DeviceDataset.from_arrays(pts, np.arange(M) if labels else None, **kw), pts


def test_loader_is_a_function_of_seed_and_epoch():
    from gm3d_amd import data as D
    ds, _ = _dataset(npoints=16, normalize=True)
    runs = []
    for epoch in (3, 3, 4):
        loader = D.DeviceLoader(ds, 4, seed=11)
        loader.set_epoch(epoch)
        assert len(loader) == 2
        runs.append(list(loader))
        assert len(runs[-1]) == 2 and all(b.shape == (4, 16, 3) and b.is_cuda for b in runs[-1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert not any(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    loader.set_epoch(3)                                        # the same loader, set back: the same batches again
    assert all(torch.equal(a, b) for a, b in zip(runs[0], list(loader)))
    assert runs[0][0].data_ptr() != runs[0][1].data_ptr()      # fresh tensors, no ring
    state = torch.cuda.get_rng_state()
    list(loader)
    assert torch.equal(state, torch.cuda.get_rng_state())      # the default generator is left alone


def test_loader_labels_belong_to_their_clouds():
    from gm3d_amd import data as D
    ds, pts = _dataset(labels=True, normalize=False, shuffle_points=False, name="ModelNet")
    loader = D.DeviceLoader(ds, 3, drop_last=False, seed=2)
    loader.set_epoch(1)
    seen = []
    for name, kind, (points, labels) in loader:
        assert name == "ModelNet" and kind == "sample" and labels.dtype == torch.int64 and labels.is_cuda
        assert torch.equal(points.cpu(), torch.from_numpy(pts[labels.cpu().numpy()]))
        seen += labels.tolist()
    assert len(loader) == 4 and seen == loader.order() and sorted(seen) == list(range(10))


def test_two_ranks_take_disjoint_halves():
    from gm3d_amd import data as D
    ds, _ = _dataset(labels=True, normalize=False, shuffle_points=False)
    got = []
    for rank in (0, 1):
        loader = D.DeviceLoader(ds, 5, seed=7, rank=rank, world=2)
        loader.set_epoch(2)
        got.append([int(v) for _, _, (_, labels) in loader for v in labels.tolist()])
    one = D.DeviceLoader(ds, 5, seed=7, rank=0, world=1)
    one.set_epoch(2)
    order = [int(v) for _, _, (_, labels) in one for v in labels.tolist()]
    assert got[0] == order[0::2] and got[1] == order[1::2]
    assert not set(got[0]) & set(got[1]) and sorted(got[0] + got[1]) == list(range(10))


def test_from_npy_files(tmp_path):
    from gm3d_amd import data as D
    pts = np.random.RandomState(9).uniform(-1, 1, (3, 40, 3)).astype(np.float32)
    paths = []
    for i, p in enumerate(pts):
        paths.append(str(tmp_path / ("c%d.npy" % i)))
        np.save(paths[-1], p)
    ds = D.DeviceDataset.from_npy_files(paths, npoints=8)
    assert len(ds) == 3 and ds.npoints == 8 and torch.equal(ds.points.cpu(), torch.from_numpy(pts))


# --------------------------------------------------------------------------- plugged into the engine
def test_plugged_into_the_point_mae_engine():
    """train_one_epoch over a DeviceLoader (8 clouds x 256 points, batch 4) against the same engine over a plain list of the batches
    the loader yields for that seed: per-step losses bit-equal.  Both runs start from the same model and the same default-generator
    state (augmentation, masking and DropPath draw from it; the loader must not)."""
    from gm3d_amd import data as D
    from gm3d_amd import engine_pretrain_point_mae as EP
    from tests.test_gpu_point_mae_pretrain import _args, _model
    pts = np.random.RandomState(77).randn(8, 256, 3).astype(np.float32)
    ds = D.DeviceDataset.from_arrays(pts, normalize=True)

    def loader():
        ld = D.DeviceLoader(ds, 4, seed=5)
        ld.set_epoch(1)
        return ld

    ready = [b.clone() for b in loader()]
    assert len(ready) == 2 and ready[0].shape == (4, 256, 3)
    losses = []
    for feed in (loader(), ready):
        m = _model()
        opt = EP.build_optimizer(m)
        torch.manual_seed(123)
        st = EP.train_one_epoch(m, feed, opt, "cuda", 1, _args(), print_freq=100)
        losses.append(st["step_losses"])
    assert len(losses[0]) == 2 and all(math.isfinite(v) for v in losses[0])
    assert losses[0] == losses[1]


# --------------------------------------------------------------------------- unwritten memory
@pytest.mark.parametrize("pattern", ["nan", "+inf", "-inf"])
def test_no_result_depends_on_unwritten_memory(tmp_path, pattern):
    """Every allocation of gm3d_amd/data.py filled with NaN / +inf / -inf (tests/poison.py) before the kernel or the copies write it:
    the dataset read from .npy files, the batch and the index output are the same bits as without.  The sites stay recorded in
    poison.SITES: they count as reached for the coverage condition of the poison modules, which run after this one."""
    from gm3d_amd import data as D
    from tests import poison
    rng = np.random.RandomState(3)
    pts = rng.uniform(-1, 1, (3, 100, 3)).astype(np.float32)
    paths = []
    for i, p in enumerate(pts):
        paths.append(str(tmp_path / ("c%d.npy" % i)))
        np.save(paths[-1], p)
    keys = torch.from_numpy(rng.uniform(0, 1, (2, 100)).astype(np.float32)).cuda()
    idx = torch.tensor([2, 0], device="cuda")

    def run():
        ds = D.DeviceDataset.from_npy_files(paths, npoints=37, normalize=True)
        res = [ds.points]
        for normalize in (True, False):
            res += list(D.sample_normalize(ds.points, idx, keys, 37, normalize, return_idx=True))
        return [r.cpu() for r in res]

    want = run()
    with poison.poisoned(pattern) as ps:
        got = run()
    assert ps.recorded >= 5 and len(ps.sites) == 3, ps.sites
    assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(want, got))
    assert torch.equal(want[0], torch.from_numpy(pts))

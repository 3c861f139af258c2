"""CPU: the reconstruction pass without a GPU -- every host-side guard of gm3d_reconstruct_assemble, what "the reference's layout"
means on the committed fixture alone (tests/golden/reconstruct.npz, made by the reference's own Point_MAE.forward(vis=True)), and
the tester (gm3d_amd/runner.py) with a stub model."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
ONE = ctypes.c_void_p(16)      # never dereferenced: a guard fails (or the empty batch returns) first
CASES = ("rand_b1", "rand_b2", "block_b2")


def _call(**kw):
    from gm3d_amd._capi import lib
    a = dict(pred=ONE, pred_bstride=38 * 96, neighborhood=ONE, center=ONE, vis_ids=ONE, vis_stride=26, mask_ids=ONE, mask_stride=38,
             B=0, G=64, k=32, V=26, M=38, layout=0, dense=ONE, full_center=ONE, dtype=0)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.gm3d_reconstruct_assemble(a["pred"], a["pred_bstride"], a["neighborhood"], a["center"], a["vis_ids"], a["vis_stride"],
                                         a["mask_ids"], a["mask_stride"], a["B"], a["G"], a["k"], a["V"], a["M"], a["layout"],
                                         a["dense"], a["full_center"], a["dtype"], None)


# --------------------------------------------------------------------------- guards (all before any launch)
def test_empty_batch_is_ok_and_launches_nothing():
    from gm3d_amd._capi import GM3D_OK
    assert _call() == GM3D_OK
    assert _call(layout=1, dtype=1) == GM3D_OK
    assert _call(G=7, k=5, V=3, M=4, vis_stride=3, mask_stride=4, pred_bstride=60) == GM3D_OK


@pytest.mark.parametrize("name", ["neighborhood", "center", "dense", "full_center", "vis_ids", "mask_ids", "pred"])
def test_null_pointer(name):
    from gm3d_amd._capi import GM3D_EINVAL
    assert _call(**{name: None}) == GM3D_EINVAL
    assert _call(**{name: None, "B": 2}) == GM3D_EINVAL


def test_nothing_visible_or_nothing_masked_needs_no_pointer_for_it():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_OK
    assert _call(V=0, M=64, vis_ids=None, vis_stride=0, mask_stride=64, pred_bstride=64 * 96) == GM3D_OK
    assert _call(V=64, M=0, vis_stride=64, mask_ids=None, mask_stride=0, pred=None, pred_bstride=0) == GM3D_OK
    assert _call(V=64, M=0, vis_stride=64, mask_ids=None, mask_stride=0, pred=None, pred_bstride=0, dense=None) == GM3D_EINVAL


@pytest.mark.parametrize("kw", [dict(V=25), dict(M=39), dict(V=-1, M=65, mask_stride=65, pred_bstride=65 * 96), dict(V=65, M=-1, vis_stride=65),
                                dict(k=0), dict(k=-3), dict(G=0, V=0, M=0), dict(G=-64), dict(B=-1), dict(layout=2), dict(layout=-1),
                                dict(dtype=2), dict(dtype=-1), dict(vis_stride=25), dict(mask_stride=37), dict(pred_bstride=38 * 96 - 1)],
                         ids=str)
def test_bad_shape_layout_or_dtype(kw):
    from gm3d_amd._capi import GM3D_EINVAL
    assert _call(**kw) == GM3D_EINVAL
    assert _call(**dict({"B": 2}, **kw)) == GM3D_EINVAL


def test_index_range():
    """B * G * k * 3 >= 2^31 is refused: patch and row indices are ints.  (The last accepted value would launch.)"""
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED
    B = -(-2 ** 31 // (64 * 32 * 3))
    assert B * 64 * 32 * 3 >= 2 ** 31 > (B - 1) * 64 * 32 * 3
    assert _call(B=B) == GM3D_EUNSUPPORTED
    assert _call(B=2 ** 31 - 1) == GM3D_EUNSUPPORTED
    assert _call(B=B, layout=5) == GM3D_EINVAL          # an invalid argument is reported first


def test_op_refuses_cpu_tensors():
    from gm3d_amd import ops
    nb, c = torch.zeros(1, 4, 2, 3), torch.zeros(1, 4, 3)
    ids = torch.arange(4).view(1, 4)
    with pytest.raises(RuntimeError):
        ops.reconstruct_assemble(torch.zeros(1, 2, 6), nb, c, ids[:, :2], ids[:, 2:])


# --------------------------------------------------------------------------- the reference's layout, on the fixture alone
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "reconstruct.npz"))


@pytest.fixture(scope="module")
def groups(fx):
    """FPS centres and KNN patches of the fixture's clouds by the CPU oracle (what the generator's stand-ins called)."""
    from oracle import model_ref as R
    pts = torch.from_numpy(fx["pts"])
    neighborhood, center, _ = R.Group(64, 32)(pts)
    return pts, neighborhood, center


@pytest.mark.parametrize("name", CASES)
def test_fixture_layout(fx, groups, name):
    """ret1 = [all clouds' visible patches | all clouds' rebuilt patches], each cloud's patches in ascending group order;
    full_center = [all MASKED centres | all visible centres].  Regrouped by the recorded mask, the visible rows of every cloud are
    (pts[knn] - centre) + centre of exactly the unmasked groups, bit for bit."""
    from gm3d_amd import runner
    _, neighborhood, center = groups
    mask = torch.from_numpy(fx[name + "/mask"])
    B, G = mask.shape
    k = 32
    M = int(mask[0].sum())
    V = G - M
    ret2, rebuilt, fc = (torch.from_numpy(fx[name + "/" + n]) for n in ("ret2", "rebuilt", "full_center"))
    assert tuple(ret2.shape) == (B * V * k, 3) and tuple(rebuilt.shape) == (B * M * k, 3) and tuple(fc.shape) == (B * G, 3)
    assert bool((mask.sum(1) == M).all()) and M == 38
    ret1 = torch.cat([ret2, rebuilt]).unsqueeze(0)
    dense, vis = runner.split_flat(ret1, ret1[:, :B * V * k], B)
    assert tuple(dense.shape) == (B, G * k, 3) and tuple(vis.shape) == (B, V * k, 3)
    for b in range(B):
        nb, c = neighborhood[b], center[b]
        want = (nb[~mask[b]] + c[~mask[b]].unsqueeze(1)).reshape(V * k, 3)
        assert torch.equal(vis[b], want) and torch.equal(dense[b, :V * k], want)
        assert torch.equal(dense[b, V * k:], rebuilt[b * M * k:(b + 1) * M * k])
        assert torch.equal(fc[b * M:(b + 1) * M], c[mask[b]])                         # masked centres first ...
        assert torch.equal(fc[B * M + b * V:B * M + (b + 1) * V], c[~mask[b]])        # ... then the visible ones
    assert 0 < float(fx[name + "/ac_err"]) < 0.05 and np.isfinite(float(fx[name + "/loss"]))


def test_fixture_cases_share_their_first_cloud(fx):
    assert tuple(fx["pts"].shape) == (2, 1024, 3)
    assert tuple(fx["rand_b1/mask"].shape) == (1, 64) and tuple(fx["block_b2/start"].shape) == (2,)
    assert os.path.getsize(os.path.join(GOLD, "reconstruct.npz")) < 200 * 1024


# --------------------------------------------------------------------------- the tester with a stub model
class Stub(torch.nn.Module):
    """vis=True of a "model" with 5 visible and 3 rebuilt rows per cloud, in the flat layout"""

    NV = 5

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, points, vis=False):
        assert vis and not self.training
        self.calls += 1
        B = points.shape[0]
        head, tail = points[:, :self.NV].reshape(-1, 3), points[:, self.NV:].reshape(-1, 3) * 2.0
        ret1 = torch.cat([head, tail]).unsqueeze(0)
        return ret1, ret1[:, :B * self.NV], torch.zeros(B, 3)


def _read(path, name):
    return np.loadtxt(os.path.join(path, name), delimiter=";")


def test_runner_writes_the_three_files_per_kept_cloud(tmp_path):
    from gm3d_amd import runner
    g = torch.Generator().manual_seed(3)
    clouds_ = [torch.randn(2, 8, 3, generator=g), torch.randn(1, 8, 3, generator=g), torch.randn(1, 8, 3, generator=g)]
    loader = [(["02691156", "99999999"], ["m0", "m1"], clouds_[0]), (["12345678"], ["m2"], clouds_[1]),
              (["03001627"], ["m3"], clouds_[2])]
    model = Stub().train()
    out = str(tmp_path / "vis")
    recs = runner.test(model, loader, out_dir=out)
    assert model.calls == 2 and not model.training          # the batch with no listed category never reaches the model
    assert sorted(os.listdir(out)) == ["02691156_0", "03001627_3"]
    assert [(r["idx"], r["taxonomy_id"], r["model_id"], r["view"]) for r in recs] == [(0, "02691156", "m0", (90, 135)),
                                                                                     (3, "03001627", "m3", (30, -45))]
    for r, pts in zip(recs, (clouds_[0][0], clouds_[2][0])):
        assert sorted(os.listdir(r["path"])) == ["dense_points.txt", "gt.txt", "vis.txt"]
        p = pts.numpy()
        assert np.array_equal(_read(r["path"], "gt.txt").astype(np.float32), p)
        assert np.array_equal(_read(r["path"], "vis.txt").astype(np.float32), p[:5])
        assert np.array_equal(_read(r["path"], "dense_points.txt").astype(np.float32), np.concatenate([p[:5], p[5:] * 2.0]))
    # every other listed category is drawn at (0, 0); max_idx stops after the first written cloud beyond it
    recs = runner.test(model, [(["03790512", "02958343"], ["a", "b"], clouds_[0])], out_dir=str(tmp_path / "v2"), max_idx=-1)
    assert [(r["idx"], r["view"]) for r in recs] == [(0, (0, 0))]
    recs = runner.test(model, loader, out_dir=str(tmp_path / "v3"), useful_cate=("12345678",))
    assert [r["idx"] for r in recs] == [2]
    assert len(runner.USEFUL_CATE) == 11 and set(runner.VIEW_ANGLES) <= set(runner.USEFUL_CATE)


def test_split_flat_refuses_what_does_not_split():
    from gm3d_amd import runner
    with pytest.raises(ValueError):
        runner.split_flat(torch.zeros(1, 10, 3), torch.zeros(1, 5, 3), 2)

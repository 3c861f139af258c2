"""CPU: the Point-M2AE reconstruction pass without a GPU -- the library exports gm3d_reconstruct_partition, every host-side guard of
it returns its code before any launch, the aten restatement (tests/m2ae_reconstruct_ref.py) gives a hand-written result, and
runner.test_m2ae writes its ragged files from a stub result."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import m2ae_reconstruct_ref as MR

ONE = ctypes.c_void_p(16)      # never dereferenced: a guard fails (or the empty batch returns) first
LIMIT = 8192                   # the largest G (include/gm3d.h)
POINTERS = ("neighborhood", "center", "masked", "dense", "full_center", "order", "n_visible")


def _call(**kw):
    from gm3d_amd._capi import lib
    a = dict(pred=ONE, neighborhood=ONE, center=ONE, masked=ONE, B=0, G=256, k=8, dtype=0, dense=ONE, full_center=ONE, order=ONE,
             n_visible=ONE)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.gm3d_reconstruct_partition(a["pred"], a["neighborhood"], a["center"], a["masked"], a["B"], a["G"], a["k"], a["dtype"],
                                          a["dense"], a["full_center"], a["order"], a["n_visible"], None)


# --------------------------------------------------------------------------- the symbol and its guards (all before any launch)
def test_the_library_exports_the_entry_point():
    from gm3d_amd import _capi
    assert "gm3d_reconstruct_partition" in _capi.SIGNATURES and len(_capi.SIGNATURES["gm3d_reconstruct_partition"]) == 13
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "gm3d_reconstruct_partition")


def test_empty_batch_is_ok_and_launches_nothing():
    from gm3d_amd._capi import GM3D_OK
    assert _call() == GM3D_OK
    assert _call(dtype=1) == GM3D_OK
    assert _call(pred=None) == GM3D_OK and _call(pred=None, G=512, k=16) == GM3D_OK
    assert _call(G=1, k=1) == GM3D_OK


@pytest.mark.parametrize("name", POINTERS)
def test_null_pointer(name):
    from gm3d_amd._capi import GM3D_EINVAL
    assert _call(**{name: None}) == GM3D_EINVAL
    assert _call(**{name: None, "B": 2}) == GM3D_EINVAL
    assert _call(**{name: None, "pred": None}) == GM3D_EINVAL


@pytest.mark.parametrize("kw", [dict(G=0), dict(G=-3), dict(k=0), dict(k=-1), dict(B=-1), dict(dtype=2), dict(dtype=-1),
                                dict(dtype=2, pred=None)], ids=str)
def test_bad_shape_or_dtype(kw):
    from gm3d_amd._capi import GM3D_EINVAL
    assert _call(**kw) == GM3D_EINVAL
    if "B" not in kw:
        assert _call(**dict({"B": 2}, **kw)) == GM3D_EINVAL


def test_token_limit():
    """G = 8192 passes every guard (B = 0 returns before a launch; a NULL pointer is still reported); G = 8193 is refused."""
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_OK
    assert _call(G=LIMIT, k=1) == GM3D_OK and _call(G=LIMIT, k=1, pred=None, dtype=1) == GM3D_OK
    assert _call(G=LIMIT, k=1, order=None) == GM3D_EINVAL
    assert _call(G=LIMIT + 1, k=1) == GM3D_EUNSUPPORTED and _call(G=LIMIT + 1, k=1, B=1) == GM3D_EUNSUPPORTED
    assert _call(G=2 ** 31 - 1, k=1) == GM3D_EUNSUPPORTED
    assert _call(G=LIMIT + 1, k=0) == GM3D_EINVAL          # an invalid argument is reported first


def test_index_range():
    """B * G * k * 3 >= 2^31 is refused: the grid size and the row length are ints.  3 does not divide 2^31, so the bound is tested
    at the first product at or above it, from both sides.  (The last accepted value would launch.)"""
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED
    B = -(-2 ** 31 // (256 * 8 * 3))
    assert B * 256 * 8 * 3 >= 2 ** 31 > (B - 1) * 256 * 8 * 3
    assert _call(B=B) == GM3D_EUNSUPPORTED
    k = -(-2 ** 31 // 3)
    assert k * 3 >= 2 ** 31 > (k - 1) * 3
    assert _call(B=1, G=1, k=k) == GM3D_EUNSUPPORTED
    assert _call(B=2 ** 31 - 1) == GM3D_EUNSUPPORTED and _call(B=2 ** 31 - 1, G=LIMIT, k=2 ** 31 - 1) == GM3D_EUNSUPPORTED
    assert _call(B=B, dtype=5) == GM3D_EINVAL              # an invalid argument is reported first


def test_op_refuses_cpu_tensors():
    from gm3d_amd import ops
    nb, c, m = torch.zeros(1, 4, 2, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        ops.reconstruct_partition(torch.zeros(1, 4, 6), nb, c, m)
    with pytest.raises(RuntimeError):
        ops.reconstruct_partition(None, nb, c, m)


# --------------------------------------------------------------------------- the aten restatement, by hand
def test_helper_gives_the_hand_written_partition():
    """B = 2, G = 5, k = 1, masks [0,1,0,1,1] and [1,1,1,1,1]: slots = visible tokens ascending, then masked tokens ascending."""
    nb = torch.arange(30, dtype=torch.float32).view(2, 5, 1, 3)                  # token t of cloud b: 15b + 3t + (0, 1, 2)
    center = torch.tensor([[[100.0, 200.0, 300.0]] * 5, [[1000.0, 2000.0, 3000.0]] * 5]) + torch.arange(5.0).view(1, 5, 1) * 0.5
    pred = -torch.arange(30, dtype=torch.float32).view(2, 5, 3) - 0.25
    masked = torch.tensor([[0, 1, 0, 1, 1], [1, 1, 1, 1, 1]], dtype=torch.uint8)
    want_order = torch.tensor([[0, 2, 1, 3, 4], [0, 1, 2, 3, 4]], dtype=torch.int32)
    want_nv = torch.tensor([2, 0], dtype=torch.int32)
    rows, centres = [], []
    for b in range(2):
        for slot in range(5):
            t = int(want_order[b, slot])
            src = pred[b, t] if masked[b, t] else nb[b, t, 0]
            rows.append(src + center[b, t])
            centres.append(center[b, t])
    want_dense, want_center = torch.stack(rows).view(2, 5, 3), torch.stack(centres).view(2, 5, 3)
    for mk in (masked, masked.bool(), masked * 255, masked * 2):
        dense, fc, order, nv = MR.partition(pred, nb, center, mk)
        assert order.dtype == torch.int32 and nv.dtype == torch.int32 and dense.dtype == torch.float32
        assert torch.equal(order, want_order) and torch.equal(nv, want_nv)
        assert torch.equal(dense, want_dense) and torch.equal(fc, want_center)
    # spelled out for cloud 0: tokens 0 and 2 are visible (true patch), 1, 3, 4 rebuilt (pred)
    assert dense[0].tolist() == [[100.0, 201.0, 302.0], [107.0, 208.0, 309.0], [97.25, 196.25, 295.25], [92.25, 191.25, 290.25],
                                 [89.75, 188.75, 287.75]]
    # without pred the masked rows are the true patches; bf16 pred is widened, and NaN in rows of visible tokens is never read
    dense0, _, order0, _ = MR.partition(None, nb, center, masked)
    assert torch.equal(order0, want_order) and torch.equal(dense0, (MR._take(nb, want_order.long()) + want_center.unsqueeze(2)).view(2, 5, 3))
    poisoned = pred.clone()
    poisoned[0, 0] = poisoned[0, 2] = float("nan")
    assert torch.equal(MR.partition(poisoned, nb, center, masked)[0], want_dense)
    assert torch.equal(MR.partition(pred.bfloat16(), nb, center, masked)[0],
                       MR.partition(pred.bfloat16().float(), nb, center, masked)[0])


# --------------------------------------------------------------------------- the tester with a stub pass
class _Result:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _stub(calls, k0=2, G0=4):
    """a reconstruct_m2ae whose level 0 is the input split into G0 tokens of k0 points, cloud b with (b + calls) % (G0 + 1) visible
    tokens, and whose dense cloud is the input doubled"""
    def reconstruct_m2ae(model, points, teacher, epoch, total_epoch, bf16=False):
        assert (teacher, epoch, total_epoch, bf16) == ("T", 7, 9, False)
        B = points.shape[0]
        nv0 = torch.tensor([(b + len(calls)) % (G0 + 1) for b in range(B)], dtype=torch.int32)
        calls.append(nv0.tolist())
        return _Result(dense=points * 2.0, points0=points[:, :G0 * k0].clone(), n_visible0=nv0,
                       masks=[torch.zeros(B, G0, dtype=torch.bool)])
    return reconstruct_m2ae


def _read(path, name):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # an empty vis.txt (nothing visible) reads as an empty array
        return np.loadtxt(os.path.join(path, name), delimiter=";", ndmin=2)


def test_runner_m2ae_writes_the_three_files_per_kept_cloud(tmp_path, monkeypatch):
    from gm3d_amd import reconstruct, runner
    g = torch.Generator().manual_seed(3)
    clouds_ = [torch.randn(2, 8, 3, generator=g), torch.randn(2, 8, 3, generator=g)]
    loader = [(["02691156", "99999999"], ["m0", "m1"], clouds_[0]), (["03001627", "04379243"], ["m2", "m3"], clouds_[1])]
    calls = []
    monkeypatch.setattr(reconstruct, "reconstruct_m2ae", _stub(calls))
    out = str(tmp_path / "vis")
    recs = runner.test_m2ae(torch.nn.Identity(), "T", loader, out, 7, 9)
    assert calls == [[0, 1], [1, 2]]
    assert sorted(os.listdir(out)) == ["02691156_0", "03001627_2", "04379243_3"]
    assert [(r["idx"], r["taxonomy_id"], r["model_id"], r["view"]) for r in recs] == [
        (0, "02691156", "m0", (90, 135)), (2, "03001627", "m2", (30, -45)), (3, "04379243", "m3", (30, 30))]
    for r, pts, tokens in zip(recs, (clouds_[0][0], clouds_[1][0], clouds_[1][1]), (0, 1, 2)):
        assert os.path.basename(r["path"]) == "%s_%d" % (r["taxonomy_id"], r["idx"])
        assert sorted(os.listdir(r["path"])) == ["dense_points.txt", "gt.txt", "vis.txt"]
        p = pts.numpy()
        assert np.array_equal(_read(r["path"], "gt.txt").astype(np.float32), p)
        vis = _read(r["path"], "vis.txt").astype(np.float32)
        assert vis.shape[0] == tokens * 2                                      # ragged: k0 = 2 rows per visible level-0 token
        assert np.array_equal(vis.reshape(-1, 3), p[:tokens * 2])
        assert np.array_equal(_read(r["path"], "dense_points.txt").astype(np.float32), p * 2.0)
    # max_idx stops after the first written cloud beyond it; a batch with no listed category never reaches the pass
    del calls[:]
    recs = runner.test_m2ae(torch.nn.Identity(), "T", loader, str(tmp_path / "v2"), 7, 9, max_idx=1)
    assert [r["idx"] for r in recs] == [0, 2]
    del calls[:]
    recs = runner.test_m2ae(torch.nn.Identity(), "T", loader, str(tmp_path / "v3"), 7, 9, useful_cate=("99999999",))
    assert [r["idx"] for r in recs] == [1] and len(calls) == 1
    recs = runner.test_m2ae(torch.nn.Identity(), "T", loader, str(tmp_path / "v4"), 7, 9, useful_cate=())
    assert recs == [] and len(calls) == 1


def test_reconstruct_m2ae_needs_a_teacher_or_a_mask():
    from gm3d_amd import reconstruct as RC

    class Raw(torch.nn.Module):
        num_group = 64

    with pytest.raises(ValueError):
        RC.reconstruct_m2ae(Raw(), torch.zeros(1, 8, 3))

"""CPU: the host side of the voting evaluation (engine_finetune.validate_vote / test_vote, P/tools/runner_finetune.py:271-335,
:399-461) -- the host draws against those recorded from the reference's own run (tests/golden/vote_b4.npz), the point_all
table, and the argument checks of the two C ABI entry points (no compute calls here)."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "vote_b4.npz"))


def test_draws_reproduce_the_reference_draws(fx):
    """Seeded alike, draw_votes makes the reference's np.random calls in its order: V x [choice, B x (uniform3, uniform3)]."""
    from gm3d_amd import engine_finetune as EF
    times, npoints = int(fx["times"]), int(fx["npoints"])
    np.random.seed(int(fx["seed"]))
    for i in range(3):
        B = fx["labels%d" % i].size
        point_all = EF.vote_point_all(npoints, fx["pts%d" % i].shape[1])
        subsets, scale, shift = EF.draw_votes(np.random, point_all, npoints, times, B)
        assert subsets.dtype == np.int64 and scale.dtype == np.float32 and shift.dtype == np.float32
        assert np.array_equal(subsets, fx["subsets%d" % i])
        assert np.array_equal(scale, fx["xyz1_%d" % i].astype(np.float32))       # torch.from_numpy(xyz1).float()
        assert np.array_equal(shift, fx["xyz2_%d" % i].astype(np.float32))
    # a RandomState draws the same stream as the seeded module
    rs = np.random.RandomState(int(fx["seed"]))
    subsets, scale, _ = EF.draw_votes(rs, 1200, npoints, times, 4)
    assert np.array_equal(subsets, fx["subsets0"]) and np.array_equal(scale, fx["xyz1_0"].astype(np.float32))


def test_point_all_table():
    from gm3d_amd import engine_finetune as EF
    assert EF.vote_point_all(1024, 8192) == 1200
    assert EF.vote_point_all(1024, 1100) == 1100            # capped at the cloud size
    assert EF.vote_point_all(2048, 8192) == 2400            # the product's extra entry
    assert EF.vote_point_all(4096, 10000) == 4800
    assert EF.vote_point_all(8192, 8192) == 8192
    for n in (512, 1000, 16384):
        with pytest.raises(NotImplementedError):
            EF.vote_point_all(n, 8192)


class _Tiny(torch.nn.Module):
    cls_dim = 40

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 3)


@pytest.mark.parametrize("graphed", [True, False])
def test_unknown_npoints_raises_and_restores_mode(graphed):
    from gm3d_amd import engine_finetune as EF
    m = _Tiny().train()
    loader = [(None, None, (torch.zeros(2, 2048, 3), torch.zeros(2, dtype=torch.long)))]
    with pytest.raises(NotImplementedError):
        EF.validate_vote(m, loader, "cpu", npoints=512, graphed=graphed)
    assert m.training


def test_vote_entry_points_check_arguments_before_any_launch():
    from gm3d_amd._capi import lib, GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_F32, GM3D_BF16
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fail first
    # gm3d_vote_sample(points, fps_idx, subsets, scale, shift, B, N0, point_all, npoints, V, out, stream)
    assert lib.gm3d_vote_sample(None, one, one, one, one, 4, 2048, 1200, 1024, 10, one, None) == GM3D_EINVAL
    assert lib.gm3d_vote_sample(one, one, one, one, one, 4, 2048, 1200, 1024, 10, None, None) == GM3D_EINVAL
    assert lib.gm3d_vote_sample(one, one, one, one, one, 4, 2048, 1200, 1300, 10, one, None) == GM3D_EINVAL   # npoints > point_all
    assert lib.gm3d_vote_sample(one, one, one, one, one, 4, 1000, 1200, 1024, 10, one, None) == GM3D_EINVAL   # point_all > N0
    assert lib.gm3d_vote_sample(one, one, one, one, one, 0, 2048, 1200, 1024, 10, one, None) == GM3D_EINVAL

    def tail(x=one, V=10, B=4, T=65, C=384, cls_dim=40, heads=None, labels=one, mean=one, pred=one, correct=one, dtype=GM3D_F32):
        hp = heads if heads is not None else [one] * 14
        return lib.gm3d_cls_tail_vote(x, V, B, T, C, *hp, cls_dim, 1e-5, labels, mean, pred, correct, None, dtype, None)

    assert tail(x=None) == GM3D_EINVAL
    assert tail(heads=[one] * 6 + [None] + [one] * 7) == GM3D_EINVAL
    assert tail(labels=None) == GM3D_EINVAL and tail(correct=None) == GM3D_EINVAL and tail(pred=None) == GM3D_EINVAL
    assert tail(B=0) == GM3D_EINVAL and tail(V=0) == GM3D_EINVAL
    assert tail(C=256) == GM3D_EUNSUPPORTED
    assert tail(cls_dim=257) == GM3D_EUNSUPPORTED
    assert tail(T=1) == GM3D_EUNSUPPORTED
    assert tail(V=17) == GM3D_EUNSUPPORTED
    assert tail(dtype=7) == GM3D_EUNSUPPORTED
    assert tail(x=ctypes.c_void_p(24), dtype=GM3D_BF16) == GM3D_EUNSUPPORTED        # rows are read 16 bytes at a time

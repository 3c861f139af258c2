"""CPU: device-resident datasets (include/gm3d.h gm3d_sample_normalize, gm3d_amd/data.py) -- the entry point refuses every shape
outside its contract on the host, with no launch, and DeviceLoader's epoch order and length are those of the reference's
DistributedSampler + DataLoader."""
import ctypes

import pytest
import torch
from torch.utils.data import DistributedSampler


def test_argument_errors_come_back_without_a_launch():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, lib
    p = ctypes.c_void_p(16)          # never dereferenced: the checks fail first
    f = lib.gm3d_sample_normalize
    #            data cloud_idx keys B  M  N0  num normalize out idx_out stream
    assert f(None, p, p, 2, 4, 64, 16, 1, p, None, None) == GM3D_EINVAL
    assert f(p, None, p, 2, 4, 64, 16, 1, p, None, None) == GM3D_EINVAL
    assert f(p, p, None, 2, 4, 64, 16, 1, p, None, None) == GM3D_EINVAL
    assert f(p, p, p, 2, 4, 64, 16, 1, None, p, None) == GM3D_EINVAL
    assert f(p, p, p, 2, 4, 64, 0, 1, p, None, None) == GM3D_EINVAL           # num < 1
    assert f(p, p, p, 2, 4, 64, -3, 0, p, None, None) == GM3D_EINVAL
    assert f(p, p, p, 2, 4, 64, 65, 1, p, None, None) == GM3D_EINVAL          # num > N0
    assert f(p, p, p, 0, 4, 64, 16, 1, p, None, None) == GM3D_EINVAL          # B < 1
    assert f(p, p, p, 2, 0, 64, 16, 1, p, None, None) == GM3D_EINVAL          # M < 1
    assert f(p, p, p, 2, 4, 0, 1, 1, p, None, None) == GM3D_EINVAL            # N0 < 1
    assert f(p, p, p, 2, 4, 64, 16, 2, p, None, None) == GM3D_EINVAL          # normalize is 0 or 1
    assert f(p, p, p, 2, 4, 8193, 16, 1, p, None, None) == GM3D_EUNSUPPORTED  # N0 > 8192
    assert f(p, p, p, 2, 4, 100000, 100000, 0, p, p, None) == GM3D_EUNSUPPORTED


def test_wrapper_refuses_cpu_tensors():
    from gm3d_amd import data as D
    with pytest.raises(RuntimeError):
        D.sample_normalize(torch.zeros(2, 8, 3), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 8), 4, True)
    with pytest.raises(RuntimeError):
        D.DeviceDataset(torch.zeros(2, 8, 3), device="cpu")


class _Clouds:
    """What DeviceLoader needs of a dataset for its order and length."""

    def __init__(self, M):
        self.M = M

    def __len__(self):
        return self.M


@pytest.mark.parametrize("M", [10, 11, 7])
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_order_is_the_distributed_samplers(M, world, shuffle):
    from gm3d_amd import data as D
    seen = []
    for rank in range(world):
        sampler = DistributedSampler(range(M), world, rank, shuffle, 13, drop_last=False)
        loader = D.DeviceLoader(_Clouds(M), 2, shuffle=shuffle, seed=13, rank=rank, world=world)
        for epoch in (0, 5):
            sampler.set_epoch(epoch)
            loader.set_epoch(epoch)
            assert loader.order() == list(sampler) and len(loader.order()) == len(sampler) == loader.num_samples
            seen.append(loader.order())
    if shuffle:
        assert seen[0] != seen[1]                             # two epochs differ


def test_more_ranks_than_clouds_pads_like_the_sampler():
    from gm3d_amd import data as D
    for rank in range(5):
        sampler = DistributedSampler(range(2), 5, rank, True, 3, drop_last=False)
        sampler.set_epoch(1)
        assert D.epoch_order(2, 1, True, 3, rank, 5) == list(sampler)


def test_len_with_and_without_drop_last():
    from gm3d_amd import data as D
    assert len(D.DeviceLoader(_Clouds(10), 4, rank=0, world=1)) == 2
    assert len(D.DeviceLoader(_Clouds(10), 4, drop_last=False, rank=0, world=1)) == 3
    assert len(D.DeviceLoader(_Clouds(12), 4, drop_last=False, rank=0, world=1)) == 3
    assert len(D.DeviceLoader(_Clouds(11), 4, rank=1, world=2)) == 1           # 6 per rank
    assert len(D.DeviceLoader(_Clouds(11), 4, drop_last=False, rank=1, world=2)) == 2
    assert len(D.DeviceLoader(_Clouds(3), 4, rank=0, world=1)) == 0
    with pytest.raises(ValueError):
        D.DeviceLoader(_Clouds(3), 4, rank=2, world=2)

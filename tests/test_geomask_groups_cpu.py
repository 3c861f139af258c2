"""CPU: num_group of the GeoMask3D Point-MAE (models_mae_learn_loss.MaskedAutoencoderViT) is the caller's, 1..512; the CPU path of
generate_mask at 128 groups against the oracle's under a shared noise ranking; csrc/guided.hip is part of the gfx950 library."""
import os
import sys

import pytest
import torch

from oracle import model_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoiseRng:
    """stands in for np.random in the oracle's generate_mask: shuffles by the ranking of a given noise (tests/test_gpu_model.py)"""

    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def shuffle(self, arr):
        n = self.noise[self.i][torch.from_numpy(arr)]
        arr[:] = arr[torch.argsort(n).numpy()]
        self.i += 1


@pytest.mark.parametrize("G", [1, 64, 128, 256, 512])
def test_constructor_and_factory_take_num_group(G):
    from gm3d_amd import models_mae_learn_loss as M
    for make in (M.MaskedAutoencoderViT, M.mae_vit_base_patch16_dec512d8b):
        m = make(num_group=G)
        assert m.num_group == G and m.group_divider.num_group == G
        assert m.group_size == 32 and m.group_divider.group_size == 32


def test_default_is_the_reference_literal():
    from gm3d_amd import models_mae_learn_loss as M
    m = M.mae_vit_base_patch16_dec512d8b()
    assert m.num_group == 64 and m.group_divider.num_group == 64


@pytest.mark.parametrize("G", [0, 513, -1, 64.5])
def test_num_group_out_of_range_is_a_value_error(G):
    from gm3d_amd import models_mae_learn_loss as M
    with pytest.raises(ValueError):
        M.MaskedAutoencoderViT(num_group=G)
    with pytest.raises(ValueError):
        M.mae_vit_base_patch16_dec512d8b(num_group=G)


@pytest.mark.parametrize("epoch", [0, 200, 399])
def test_cpu_generate_mask_at_128_groups_equals_the_oracle(epoch):
    """L = 128, ratio 0.6: the argsort / scatter formulation of the package on the CPU == the oracle's per-cloud shuffle, both driven by
    the same noise ranking (distinct loss_pred and noise: no tie to resolve)."""
    from gm3d_amd import models_mae_learn_loss as M
    B, L = 5, 128
    g = torch.Generator().manual_seed(epoch + 1)
    lp, noise = torch.randn(B, L, generator=g), torch.rand(B, L, generator=g)
    m = M.mae_vit_base_patch16_dec512d8b(num_group=L)
    om = R.PointMAEGM3D(num_group=L)
    got = m.generate_mask(lp, 0.6, epoch=epoch, total_epoch=400, noise=noise)
    want = om.generate_mask(lp, 0.6, epoch=epoch, total_epoch=400, rng=_NoiseRng(noise), noise=noise)
    assert torch.equal(got, want)
    assert int((got == 0).sum()) == B * int(L * 0.4)


def test_guided_kernels_are_in_the_gfx950_library():
    """build() cross-compiles csrc/guided.hip for gfx950 and links it: both kernels are in the library's device code, the C ABI has
    gained no symbol for them, and the limits of the entry points in front of them are checked on the host."""
    import ctypes
    from gm3d_amd import build
    assert "guided.hip" in build.SOURCES and build.ARCH == "gfx950"
    path = build.build()
    blob = open(path, "rb").read()
    for kernel in (b"mask_select_wide_kernel", b"rank_loss_wide_kernel", b"mask_select_kernel", b"rank_loss_kernel"):
        assert kernel in blob, kernel
    lib = ctypes.CDLL(path)
    assert not hasattr(lib, "gm3d_mask_select_wide") and not hasattr(lib, "gm3d_rank_loss_wide")
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, lib as capi
    one = ctypes.c_void_p(16)      # never dereferenced: the shape check fails first
    assert capi.gm3d_mask_select_b(one, one, 1, 513, 205, 10, one, None, one, one, 513, None) == GM3D_EUNSUPPORTED
    assert capi.gm3d_mask_select_b(one, one, 1, 512, 500, 13, one, None, one, one, 512, None) == GM3D_EINVAL      # keep + forced > L
    assert capi.gm3d_mask_select_b(one, one, 1, 200, 80, 10, one, None, one, one, 199, None) == GM3D_EINVAL       # pitch < L
    assert capi.gm3d_mask_select_b(one, one, 0, 200, 80, 10, one, None, one, one, 200, None) == 0                  # B = 0: nothing launched
    assert capi.gm3d_rank_loss(one, one, 1, 513, one, one, None) == GM3D_EUNSUPPORTED
    assert capi.gm3d_rank_loss_tail(one, 600, one, 1, 513, one, one, one, one, None) == GM3D_EUNSUPPORTED
    assert capi.gm3d_rank_loss_tail(one, 100, one, 1, 200, one, one, one, one, None) == GM3D_EINVAL                # ldp < M


def test_no_lds_access_in_flight_at_a_barrier_in_guided_hip():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import barrier_audit
    assert barrier_audit.audit([os.path.join(ROOT, "gm3d_amd", "csrc", "guided.hip")]) == []

"""The Python routing predicates against the C guards they restate.

Each predicate gets shapes and layouts on both sides of every condition it tests.  Where it says yes, the kernel it routes to must
return GM3D_OK (the public op raises Gm3dError otherwise); either way the public op must match a torch reference at the bar of its
existing test.  A predicate stricter than its guard only costs a fallback; a looser one would raise inside training.

Found looser than the guard and tightened: gemm.supported and gemm.ragged_supported (no w.stride(0) >= K: a weight with expanded
rows), gemm.wgrad_supported (no ldy >= N, ldx >= K), heads.group_max_supported (C = 0 accepted; chan_ok needs C >= 8).
Stricter than the guard, kept: gemm.supported / ragged_supported / dma_supported / wgrad_supported require 16-byte aligned operands
(the TN guard does not); gemm.supported requires N % 128 and K % 64 where the guard also takes the ragged form; ws_supported /
pool16_supported / ws_bn_supported require M >= 32768 (a speed choice); heads.patch_chamfer_loss_supported requires pred rows
of exactly 96 contiguous values.  Equal: heads.layer_norm_supported, heads.bn_bcast_supported, attention.qkv_supported.
"""
from types import SimpleNamespace

import pytest
import torch


def _guard_ok(rc):
    from gm3d_amd._capi import GM3D_OK
    return rc == GM3D_OK


# ------------------------------------------------------------------ CPU: the predicates that are pure shape tests, against the guard
def test_layer_norm_predicate_equals_add_ln_guard():
    """heads.layer_norm_supported(x, C) == gm3d_add_ln_fwd's shape guard, for every C (R = 0: the guard runs, nothing launches)."""
    import ctypes
    from gm3d_amd import heads
    from gm3d_amd._capi import lib
    one = ctypes.c_void_p(16)
    for dt, dt_id in ((torch.float32, 0), (torch.bfloat16, 1)):
        x = SimpleNamespace(is_cuda=True, dtype=dt)
        for C in range(-4, 1100):
            guard = _guard_ok(lib.gm3d_add_ln_fwd(one, None, None, None, 1, None, one, one, 1e-5, None, one, one, one, 0, C, dt_id, None))
            assert heads.layer_norm_supported(x, C) == guard, (dt, C)


# ------------------------------------------------------------------ GPU: the GEMM predicates, their kernels and the public op
def _layouts(M, N, K, g):
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).bfloat16()
    xpad = torch.zeros(M, K + 8, device="cuda", dtype=torch.bfloat16)
    xpad[:, :K] = x
    xodd = torch.zeros(M, K + 4, device="cuda", dtype=torch.bfloat16)
    xodd[:, :K] = x
    xoff = torch.zeros(M * K + 8, device="cuda", dtype=torch.bfloat16)
    xoff[4:4 + M * K] = x.flatten()
    return {
        "dense": (x, w),
        "lda=K+8": (xpad[:, :K], w),                            # aligned pitch: accepted
        "lda=K+4": (xodd[:, :K], w),                            # pitch not a multiple of 8: refused by the guard
        "x+8B": (xoff[4:4 + M * K].view(M, K), w),             # 8-byte offset: the predicates want 16-byte operands
        "w expanded": (x, w[:1].expand(N, K)),                  # ldw = 0 < K: refused by the guard
    }


def _check_product(y, x, w):
    ref = x.float() @ w.float().t()
    err = (y.float() - ref).abs()
    assert float((err / (ref.abs() + 1.0)).max()) <= 6e-3


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(64, 128, 64), (48, 256, 512), (40, 136, 72), (32, 96, 64), (64, 192, 384), (33, 128, 8),
                                   (64, 120, 64)])
def test_gemm_predicates_route_to_accepting_kernels(M, N, K):
    from gm3d_amd import gemm
    g = torch.Generator(device="cuda").manual_seed(M * N + K)
    for name, (x, w) in _layouts(M, N, K, g).items():
        s, r, d = gemm.supported(x, w), gemm.ragged_supported(x, w), gemm.dma_supported(x, w)
        assert not s or r, name                           # the tiled form is a special case of the ragged one
        if name in ("lda=K+4", "w expanded"):
            assert not (s or r or d), name
        if s or r:
            _check_product(gemm.linear_tn(x, w), x, w)    # raises if the library refuses what the predicate accepted
        if d:
            _check_product(gemm.linear_tn_dma(x, w, bm=gemm.dma_bm(M)), x, w)
        _check_product(gemm.mm(x, w), x, w)               # the public op, whatever it routes to


@pytest.mark.gpu
@pytest.mark.parametrize("R,N,K", [(64, 128, 128), (96, 136, 72), (48, 128, 128), (64, 8, 16)])
def test_wgrad_predicate_routes_to_accepting_kernel(R, N, K):
    from gm3d_amd import gemm
    g = torch.Generator(device="cuda").manual_seed(R + N + K)
    dy = torch.randn(1, R, N, device="cuda", generator=g).bfloat16()
    x = torch.randn(1, R, K, device="cuda", generator=g).bfloat16()
    cases = {"dense": (dy, x), "dy rows expanded": (dy[:, :1].expand(1, R, N), x), "x rows expanded": (dy, x[:, :1].expand(1, R, K))}
    for name, (a, b) in cases.items():
        ok = gemm.wgrad_supported(a, b)
        assert ok == (name == "dense" and R % 32 == 0), name
        want = torch.bmm(a.float().transpose(1, 2), b.float())
        if ok:
            got = gemm.wgrad_nt(a, b)
            assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()), name
        from gm3d_amd import embed
        got = embed.splitk_wgrad(a[0], b[0])                      # the public op: routed by the predicate
        bar = 2e-5 if ok else 2.0 ** -8                           # torch's bf16 bmm fallback rounds its result to bf16
        assert float((got.float() - want[0]).abs().max()) <= bar * float(want.abs().max()), name


@pytest.mark.gpu
@pytest.mark.parametrize("C", [96, 512, 100])
def test_layer_norm_predicate_and_op(C):
    from gm3d_amd import heads
    x = (torch.randn(37, C, device="cuda") * 1.5).requires_grad_(True)
    w, b = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.2
    assert heads.layer_norm_supported(x, C)
    h = heads.LayerNormFn.apply(x, w, b, 1e-5, torch.float32)
    ref = torch.nn.functional.layer_norm(x.detach().double(), (C,), w.double(), b.double(), 1e-5)
    assert float((h.double() - ref).abs().max()) <= 2e-6 * max(1.0, float(ref.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("C,K", [(8, 1), (1024, 32), (96, 255)])
def test_group_max_predicate_and_op(C, K):
    from gm3d_amd import heads
    x = torch.randn(5, K, C, device="cuda").requires_grad_(True)
    assert heads.group_max_supported(x)
    assert torch.equal(heads.GroupMaxFn.apply(x), x.detach().amax(1))


# ------------------------------------------------------------------ GPU: the dispatcher's tails and the one weight-gradient entry
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(33, 96, 72), (64, 128, 64)])
def test_fp32_products_are_the_library_s_own_without_f32_own(M, N, K):
    from gm3d_amd import gemm
    assert gemm.F32_OWN is False
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x, dy = torch.randn(M, K, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g)
    assert gemm.route(x, w) == ("lib", {})
    assert torch.equal(gemm.mm(x, w), x @ w.t())
    assert torch.equal(gemm.mm_nn(dy, w), dy @ w)


@pytest.mark.gpu
def test_linear_bias_fn_fp32_forward_is_addmm():
    from gm3d_amd import heads
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(40, 384, device="cuda", generator=g)
    w, b = torch.randn(96, 384, device="cuda", generator=g) / 20, torch.randn(96, device="cuda", generator=g)
    assert torch.equal(heads.LinearBiasFn.apply(x, w, b, torch.float32), torch.addmm(b, x, w.t()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 96, 72), (2, 64, 128, 128)])
def test_wgrad_is_the_fp32_nt_kernel_under_f32_own(shape, monkeypatch):
    from gm3d_amd import gemm
    monkeypatch.setattr(gemm, "F32_OWN", True)
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    dy = torch.randn(*shape[:-2], shape[-2], device="cuda", generator=g)
    x = torch.randn(*shape[:-2], shape[-1], device="cuda", generator=g)
    if dy.dim() == 2:
        assert torch.equal(gemm.wgrad(dy, x), gemm.wgrad_nt_f32(dy.unsqueeze(0), x.unsqueeze(0))[0])
    else:
        assert torch.equal(gemm.wgrad(dy, x), gemm.wgrad_nt_f32(dy, x))


@pytest.mark.gpu
@pytest.mark.parametrize("nb,R,N,K", [(1, 64, 128, 128), (4, 96, 136, 72), (1, 48, 128, 128)])
def test_wgrad_is_the_nt_kernel_for_bf16_and_the_library_off_its_rows(nb, R, N, K):
    from gm3d_amd import gemm
    g = torch.Generator(device="cuda").manual_seed(nb + R + N + K)
    dy = torch.randn(nb, R, N, device="cuda", generator=g).bfloat16()
    x = torch.randn(nb, R, K, device="cuda", generator=g).bfloat16()
    if R % 32 == 0:
        assert torch.equal(gemm.wgrad(dy, x), gemm.wgrad_nt(dy, x))
        assert torch.equal(gemm.wgrad(dy[0], x[0]), gemm.wgrad_nt(dy[:1], x[:1])[0])
        return
    assert not gemm.wgrad_supported(dy, x)            # R = 48: no multiple of the NT kernel's 32-row stage -> torch.bmm
    want = torch.bmm(dy.float().transpose(1, 2), x.float())
    for got in (gemm.wgrad(dy, x), gemm.wgrad(dy[0], x[0]).unsqueeze(0)):
        assert got.dtype == torch.float32
        assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())

"""-m gpu: the fp32 MFMA GEMMs (csrc/gemm_f32.hip: gm3d_gemm_tn_f32, gm3d_gemm_nt_f32) against torch.float64 products of the same
fp32 inputs.

Bound (derived, not tuned), per element: |C - C64| <= gamma * sum_k |a_ik| |w_jk| + |bias_j| * 2^-24 with
gamma = (K+1) u / (1 - (K+1) u), u = 2^-24: the standard bound of a length-K fp32 inner product summed in ANY order (K roundings of
the sum and its products, one more for the bias add).  NT: the same with R in place of K; with accumulate the previous content of
`out` is one more term of the sum (|out_prev| joins the sum of magnitudes; R + 1 roundings in all).  The fp64 reference's own error
(K * 2^-53 of the same magnitudes) is nine orders below the bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def gamma(n):
    return (n + 1) * U / (1.0 - (n + 1) * U)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _tn(a, w, bias=None, out=None):
    from gm3d_amd import gemm
    return gemm.linear_tn_f32(a, w, bias, out)


def _check_tn(c, a, w, bias, what):
    K = a.shape[1]
    ref = a.double() @ w.double().t()
    mag = a.double().abs() @ w.double().abs().t()
    bound = gamma(K) * mag
    if bias is not None:
        ref = ref + bias.double()
        bound = bound + bias.double().abs() * U
    err = (c.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound = %.3f" % (what, worst))
    assert bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("K", [1, 3, 66, 384])
@pytest.mark.parametrize("N", [1, 40, 96, 392])
@pytest.mark.parametrize("M", [1, 33, 130])
def test_tn_against_float64(M, N, K):
    a, w, bias = _randn((M, K), 1000 + M + K), _randn((N, K), 2000 + N + K), _randn((N,), 3000 + N)
    c = _tn(a, w, bias)
    assert c.shape == (M, N) and c.dtype == torch.float32
    _check_tn(c, a, w, bias, "tn %d x %d x %d" % (M, N, K))


def test_tn_null_bias():
    a, w = _randn((130, 66), 1), _randn((96, 66), 2)
    _check_tn(_tn(a, w, None), a, w, None, "tn, no bias")


def test_tn_pitches_wider_than_the_widths_and_a_column_slice_of_c():
    """A, W and C are column windows of wider buffers (odd pitches and a window start that is not 16-byte aligned: the scalar
    staging path); the columns of C's buffer on both sides of the window keep their sentinel."""
    M, N, K = 130, 96, 66
    abuf, wbuf = _randn((M, K + 7), 3), _randn((N, K + 5), 4)
    a, w = abuf[:, 3:3 + K], wbuf[:, 1:1 + K]
    bias = _randn((N,), 5)
    cbuf = torch.full((M, N + 13), 12345.0, device="cuda")
    c = cbuf[:, 6:6 + N]
    assert a.stride(0) > K and w.stride(0) > K and c.stride(0) > N
    got = _tn(a, w, bias, out=c)
    assert got.data_ptr() == c.data_ptr()
    _check_tn(c, a, w, bias, "tn, strided")
    assert bool((cbuf[:, :6] == 12345.0).all()) and bool((cbuf[:, 6 + N:] == 12345.0).all())
    # the aligned, vector-staged form of the same product has the same bits: the chain depends on K alone
    assert torch.equal(_tn(a.contiguous(), w.contiguous(), bias), c)


@pytest.mark.parametrize("M,N,K", [(8192, 1536, 384), (8192, 384, 1536)])
def test_tn_full_size(M, N, K):
    a, w, bias = _randn((M, K), 11), _randn((N, K), 12), _randn((N,), 13)
    _check_tn(_tn(a, w, bias), a, w, bias, "tn %d x %d x %d" % (M, N, K))


def _nt(dy, x, out=None, splits=None, accumulate=False):
    from gm3d_amd import gemm
    return gemm.wgrad_nt_f32(dy, x, out, splits=splits, accumulate=accumulate)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N,K", [(8, 3), (96, 384), (392, 130)])
@pytest.mark.parametrize("R", [1, 65, 4100])
@pytest.mark.parametrize("batch", [1, 3])
def test_nt_against_float64(batch, R, N, K, accumulate):
    from gm3d_amd import gemm
    dy, x = _randn((batch, R, N), 100 + R + N), _randn((batch, R, K), 200 + R + K)
    prev = _randn((batch, N, K), 300 + N + K)
    out = prev.clone()
    got = _nt(dy, x, out, accumulate=accumulate)
    assert got.data_ptr() == out.data_ptr()
    if R == 4100:
        assert gemm.nt_f32_splits(batch, R, N, K) > 1           # the slab path
    ref = dy.double().transpose(1, 2) @ x.double()
    mag = dy.double().abs().transpose(1, 2) @ x.double().abs()
    if accumulate:
        ref, mag = ref + prev.double(), mag + prev.double().abs()
    bound = gamma(R) * mag
    err = (out.double() - ref).abs()
    print("nt %d x %d x %d x %d acc=%d: worst error / bound = %.3f" % (batch, R, N, K, accumulate, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


def test_tn_is_deterministic_and_rows_do_not_depend_on_m():
    """Run twice: equal bits.  33 rows computed alone (one 64-row tile) == the same rows inside a 1100-row product (128-row tiles
    elsewhere in the grid decision) and inside the full-size 8192-row one: the order of a row's sums depends on K only."""
    a, w, bias = _randn((8192, 384), 21), _randn((1536, 384), 22), _randn((1536,), 23)
    full = _tn(a, w, bias)
    assert torch.equal(full, _tn(a, w, bias))
    small = _tn(a[:33], w, bias)
    assert torch.equal(small, _tn(a[:33], w, bias))
    assert torch.equal(small, full[:33])
    assert torch.equal(_tn(a[:1100], w, bias), full[:1100])
    assert torch.equal(_tn(a[64:64 + 130], w[:392], bias[:392]), full[64:64 + 130, :392])


@pytest.mark.parametrize("batch,R,N,K", [(1, 4100, 96, 384), (3, 4100, 392, 130)])
def test_nt_is_deterministic_and_equals_the_ascending_sum_of_its_slabs(batch, R, N, K):
    from gm3d_amd import gemm
    dy, x = _randn((batch, R, N), 31), _randn((batch, R, K), 32)
    s = gemm.nt_f32_splits(batch, R, N, K)
    assert s > 1
    got = _nt(dy, x)
    assert torch.equal(got, _nt(dy, x))
    rows = gemm.nt_f32_slab_rows(R, s)
    want = None
    for i in range(s):
        part = _nt(dy[:, i * rows:(i + 1) * rows], x[:, i * rows:(i + 1) * rows], splits=1)
        want = part if want is None else want + part
    assert torch.equal(got, want)


def test_contract_rejections_launch_nothing():
    from gm3d_amd._capi import lib, GM3D_EINVAL
    from gm3d_amd.ops import _ptr, _stream
    a, w = _randn((8, 8), 41), _randn((8, 8), 42)
    c = torch.full((8, 8), 7.0, device="cuda")
    assert lib.gm3d_gemm_tn_f32(_ptr(a), _ptr(w), None, _ptr(c), 0, 8, 8, 8, 8, 8, _stream()) == GM3D_EINVAL
    assert lib.gm3d_gemm_tn_f32(_ptr(a), _ptr(w), None, _ptr(c), 8, 8, 8, -8, 8, 8, _stream()) == GM3D_EINVAL
    assert lib.gm3d_gemm_nt_f32(_ptr(a), _ptr(w), _ptr(c), None, 1, 0, 8, 8, 8, 8, 8, 0, 0, 0, 1, 0, _stream()) == GM3D_EINVAL
    assert lib.gm3d_gemm_nt_f32(_ptr(a), _ptr(w), _ptr(c), None, 1, 8, 8, 8, 8, -8, 8, 0, 0, 0, 1, 0, _stream()) == GM3D_EINVAL
    torch.cuda.synchronize()
    assert bool((c == 7.0).all())

"""The 192-column LDS-DMA kernel (csrc/gemm_dma.hip) at the shapes where a staged K pipeline can go wrong, held BIT FOR BIT to the
tiled kernels of csrc/gemm.hip on the same operands (both promise k ascending in steps of 16 per accumulator, one bf16 rounding).
Written for a ring of several stages in flight (measured slower and dropped: profiles/NEGATIVE_RESULTS.md); every case passed on
the double-buffered kernel before it, on the ring, and on the kernel as it is: last stage peeled off the loop, the epilogue's
bias / Fpre loads requested before it is multiplied.

    K   64 (one stage: the loop does not run; fewer stages than a ring is deep), 128 / 192 (the drain path before any steady state, an
        even and an odd count of 64-column stages), 384 (the step's), 1536 (the buffers wrap many times)
    M   1, 63, 65, 130, 257: the row clamp, a partial last tile, more tiles than one at both tile heights (bm 64 / 128)
    N   384 and 192 for the plain product and the two GELU epilogues, 256 at bn = 128 and 256 for the plain product; the pool
        epilogue at M = 32 / 96, N = 384 (bn = 192 and 128)

The tiled GELU / pool kernels take whole 128-column tiles and the LDS-DMA ones whole 192-column tiles, so one problem of N = 384 is
computed by the tiled kernel once per (K, M); the 192-column launch runs on the FIRST 192 rows of the same w (bias, and columns of
f) and is compared with the first 192 columns of that result: a column depends on its own w row only.

Column-sum partials: the two kernels add the SAME fp32 values v (dF = bf16(v) is bit-equal) in different row groupings, so after
gm3d_colsum_finish the sums differ by at most 2 gamma(M) sum|v| (gemm_bf16_cases.gamma: each is within gamma(M) sum|v| of the exact
sum, any order), with |v| <= |bf16(v)| / (1 - 2^-8).

Also: the same launch 8 times gives identical bytes (a mis-counted wait shows as a race), and with every operand a window of a NaN
buffer and every destination inside a buffer of 7.0 (the helpers of tests/test_gpu_gemm_bf16_fp64.py) the results equal the calls
on contiguous copies and nothing outside the destinations changes."""
import functools

import pytest
import torch

from tests import gemm_bf16_cases as C
from tests.test_gpu_gemm_bf16_fp64 import NAN, _untouched, _window

pytestmark = pytest.mark.gpu

KS = (64, 128, 192, 384, 1536)
MS = (1, 63, 65, 130, 257)
M_TOP, N_TOP = 257, 384
POOL_MS = (32, 96)
FENCE_K, FENCE_M = 192, 65


@functools.lru_cache(maxsize=None)
def _fwd(K):
    """x (257,K), w (384,K), bias (384) on the device: made once per K, shared, never modified"""
    return tuple(t.cuda() for t in C.tn_inputs("graded", M_TOP, N_TOP, K, salt=3))


@functools.lru_cache(maxsize=None)
def _bwd(K):
    """d_o (257,K), w2t (384,K), f (257,384), bias (384)"""
    return tuple(t.cuda() for t in C.gelu_bwd_inputs(M_TOP, N_TOP, K))


@functools.lru_cache(maxsize=None)
def _pool(K, M):
    return tuple(t.cuda() for t in C.tn_inputs("graded", M, N_TOP, K, salt=11))


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if not torch.equal(a, b):
        bad = (a != b) | (a.isnan() != b.isnan())
        i = tuple(int(v) for v in bad.nonzero()[0])
        pytest.fail("%s: %d of %d elements differ, first at %s: %r against %r" % (what, int(bad.sum()), a.numel(), i, float(a[i]), float(b[i])))


@pytest.mark.parametrize("bm", (64, 128))
@pytest.mark.parametrize("K", KS)
def test_plain_product_equals_the_tiled_kernel(K, bm):
    from gm3d_amd import gemm
    x, w, b = _fwd(K)
    for M in MS:
        for bias in (None, b):
            want = gemm.linear_tn(x[:M], w, bias)
            _same(gemm.linear_tn_dma(x[:M], w, bias, bm=bm), want, "N=384 M=%d bias=%d" % (M, bias is not None))
            _same(gemm.linear_tn_dma(x[:M], w[:192], None if bias is None else bias[:192], bm=bm), want[:, :192].contiguous(),
                  "N=192 M=%d bias=%d" % (M, bias is not None))
            for bn in (128, 256):
                _same(gemm.linear_tn_dmaw(x[:M], w[:256], None if bias is None else bias[:256], bm=bm, bn=bn), want[:, :256].contiguous(),
                      "N=256 bn=%d M=%d bias=%d" % (bn, M, bias is not None))


@pytest.mark.parametrize("bm", (64, 128))
@pytest.mark.parametrize("K", KS)
def test_gelu_forward_equals_the_tiled_kernel(K, bm):
    from gm3d_amd import gemm
    x, w, b = _fwd(K)
    for M in MS:
        f0, g0 = gemm.linear_gelu(x[:M], w, b, f_out=torch.full((M, N_TOP), NAN, dtype=torch.bfloat16, device="cuda"))
        for N in (384, 192):
            f, g = gemm.linear_gelu_dma(x[:M], w[:N], b[:N], f_out=torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda"), bm=bm)
            _same(f, f0[:, :N].contiguous(), "F N=%d M=%d" % (N, M))
            _same(g, g0[:, :N].contiguous(), "G N=%d M=%d" % (N, M))
            _same(gemm.linear_gelu_dma(x[:M], w[:N], b[:N], bm=bm)[1], g, "G without F N=%d M=%d" % (N, M))


def _finish(part):
    from gm3d_amd import gemm
    from gm3d_amd.ops import _ptr, _stream, check
    rows, cols = part.shape
    db = torch.full((cols,), NAN, device="cuda")
    check(gemm.lib.gm3d_colsum_finish(_ptr(part), rows, cols, cols, _ptr(db), 0, _stream()), "gm3d_colsum_finish")
    return db


def _bwd_dma(d_o, w2t, f, b, bm):
    from gm3d_amd import gemm
    M, N = d_o.shape[0], w2t.shape[0]
    df = torch.full((M, N), NAN, dtype=torch.bfloat16, device="cuda")
    part = torch.full((-(-M // bm), N), NAN, device="cuda")
    gemm.linear_gelu_bwd_dma(d_o, w2t, f, b, df, part, bm=bm)
    return df, part


@pytest.mark.parametrize("bm", (64, 128))
@pytest.mark.parametrize("K", KS)
def test_gelu_backward_equals_the_tiled_kernel(K, bm):
    from gm3d_amd import gemm
    d_o, w2t, f, b = _bwd(K)
    for M in MS:
        df0 = torch.full((M, N_TOP), NAN, dtype=torch.bfloat16, device="cuda")
        part0 = torch.full((gemm.tile_rows(M), N_TOP), NAN, device="cuda")
        gemm.linear_gelu_bwd(d_o[:M], w2t, f[:M], b, df0, part0)
        db0 = _finish(part0)
        slack = 2.0 * C.gamma(M) * df0.double().abs().sum(0) / (1.0 - C.HALF_ULP)
        for N in (384, 192):
            df, part = _bwd_dma(d_o[:M], w2t[:N], f[:M, :N], b[:N], bm)          # f: a 192-column window of the 384-wide rows
            _same(df, df0[:, :N].contiguous(), "dF N=%d M=%d" % (N, M))
            db = _finish(part)
            assert bool(torch.isfinite(db).all()), ("column sums", N, M)
            err = (db.double() - db0[:N].double()).abs()
            print("\nDMARING colsum K=%d bm=%d M=%d N=%d worst err/bound %.3f" % (K, bm, M, N, C.worst(db, db0[:N].double(), slack[:N])))
            assert bool((err <= slack[:N]).all()), ("column sums", N, M, float((err - slack[:N]).max()))


@pytest.mark.parametrize("bm", (64, 128))
@pytest.mark.parametrize("K", KS)
def test_pool_equals_the_tiled_kernel(K, bm):
    from gm3d_amd import gemm
    for M in POOL_MS:
        x, w, b = _pool(K, M)
        for after in (False, True):
            rows0, top0, arg0 = gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=True, route=("own", {}))
            for bn in (192, 128):
                for want_rows in (True, False):
                    rows, top, arg = gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=want_rows, route=("dma", {"bm": bm, "bn": bn}))
                    what = "M=%d bn=%d after=%d rows=%d" % (M, bn, after, want_rows)
                    _same(top, top0, "pooled " + what)
                    _same(arg, arg0, "argmax " + what)
                    if want_rows:
                        _same(rows, rows0, "rows " + what)


@pytest.mark.parametrize("bm", (64, 128))
@pytest.mark.parametrize("K", (128, 1536))
def test_eight_launches_give_identical_bytes(K, bm):
    from gm3d_amd import gemm
    x, w, b = _fwd(K)
    d_o, w2t, f, bb = _bwd(K)
    px, pw, pb = _pool(K, 96)
    first = None
    for _ in range(8):
        got = (gemm.linear_tn_dma(x, w, b, bm=bm),) + tuple(gemm.linear_gelu_dma(x, w, b, f_out=torch.empty_like(f), bm=bm))
        got += _bwd_dma(d_o, w2t, f, bb, bm) + gemm.linear_pool(px, pw, pb, False, True, route=("dma", {"bm": bm, "bn": 192}))
        if first is None:
            first = got
        for a, b_ in zip(got, first):
            assert torch.equal(a.view(torch.uint8), b_.view(torch.uint8))


def _fenced(K):
    x, w, b = _fwd(K)
    _, xv = _window(x[:FENCE_M], NAN)
    _, wv = _window(w, NAN)
    bbuf = torch.full((N_TOP + 8,), NAN, device="cuda")
    bv = bbuf[4:4 + N_TOP]
    bv.copy_(b)
    return xv, wv, bv


@pytest.mark.parametrize("bm", (64, 128))
def test_nan_fence_forward(bm):
    from gm3d_amd import gemm
    x, w, b = _fwd(FENCE_K)
    xv, wv, bv = _fenced(FENCE_K)
    new = lambda: _window(torch.empty(FENCE_M, N_TOP, dtype=torch.bfloat16, device="cuda"), 7.0)
    dst, dv = new()
    gemm.linear_tn_dma(xv, wv, bv, out=dv, bm=bm)
    _same(dv.contiguous(), gemm.linear_tn_dma(x[:FENCE_M], w, b, bm=bm), "plain")
    assert _untouched(dst, dv, 7.0)
    (fd, fv), (gd, gv) = new(), new()
    gemm.linear_gelu_dma(xv, wv, bv, f_out=fv, g_out=gv, bm=bm)
    f0, g0 = gemm.linear_gelu_dma(x[:FENCE_M], w, b, f_out=torch.empty(FENCE_M, N_TOP, dtype=torch.bfloat16, device="cuda"), bm=bm)
    _same(fv.contiguous(), f0, "F")
    _same(gv.contiguous(), g0, "G")
    assert _untouched(fd, fv, 7.0) and _untouched(gd, gv, 7.0)


@pytest.mark.parametrize("bm", (64, 128))
def test_nan_fence_backward(bm):
    from gm3d_amd import gemm
    d_o, w2t, f, b = _bwd(FENCE_K)
    M = FENCE_M
    _, ov = _window(d_o[:M], NAN)
    _, wv = _window(w2t, NAN)
    _, fv = _window(f[:M], NAN)
    bbuf = torch.full((N_TOP + 8,), NAN, device="cuda")
    bv = bbuf[4:4 + N_TOP]
    bv.copy_(b)
    dst, dv = _window(torch.empty(M, N_TOP, dtype=torch.bfloat16, device="cuda"), 7.0)
    tiles = -(-M // bm)
    pbuf = torch.full((tiles + 4, N_TOP), 7.0, device="cuda")                  # the partials are read at a pitch of N: whole rows
    pv = pbuf[2:2 + tiles]
    gemm.linear_gelu_bwd_dma(ov, wv, fv, bv, dv, pv, bm=bm)
    df0, part0 = _bwd_dma(d_o[:M], w2t, f[:M], b, bm)
    _same(dv.contiguous(), df0, "dF")
    _same(pv.contiguous(), part0, "column partials")
    assert _untouched(dst, dv, 7.0)
    assert bool((pbuf[:2] == 7.0).all()) and bool((pbuf[2 + tiles:] == 7.0).all())


@pytest.mark.parametrize("bm", (64, 128))
def test_nan_fence_pool(bm):
    from gm3d_amd import gemm
    from gm3d_amd.ops import _ptr, _stream, check
    M, G = 96, 3
    x, w, b = _pool(FENCE_K, M)
    _, xv = _window(x, NAN)
    _, wv = _window(w, NAN)
    bbuf = torch.full((N_TOP + 8,), NAN, device="cuda")
    bv = bbuf[4:4 + N_TOP]
    bv.copy_(b)
    rd, rv = _window(torch.empty(M, N_TOP, dtype=torch.bfloat16, device="cuda"), 7.0)
    pd, pv = _window(torch.empty(G, N_TOP, dtype=torch.bfloat16, device="cuda"), 7.0)
    ad, av = _window(torch.empty(G, N_TOP, dtype=torch.uint8, device="cuda"), 7)
    check(gemm.lib.gm3d_gemm_tn_bf16_dma_pool(_ptr(xv), _ptr(wv), _ptr(bv), _ptr(rv), _ptr(pv), _ptr(av), M, N_TOP, FENCE_K, xv.stride(0),
                                              wv.stride(0), rv.stride(0), pv.stride(0), 0, bm, 192, _stream()), "gm3d_gemm_tn_bf16_dma_pool")
    rows0, top0, arg0 = gemm.linear_pool(x, w, b, bias_after_pool=False, want_rows=True, route=("dma", {"bm": bm, "bn": 192}))
    _same(rv.contiguous(), rows0, "rows")
    _same(pv.contiguous(), top0, "pooled")
    _same(av.contiguous(), arg0, "argmax")
    assert _untouched(rd, rv, 7.0) and _untouched(pd, pv, 7.0) and _untouched(ad, av, 7)

"""-m gpu: every bf16 MFMA GEMM kernel -- csrc/gemm.hip (unrolled, run-time-loop and ragged forms), gemm_ring.hip (128 and 96 columns),
gemm_dma.hip (`dma` / `dmaw` tile forms), gemm_ws.hip, the weight-gradient kernel gemm_nt.hip (split, big-tile, in-launch-sum and
multi-problem forms) and the GELU and pool epilogues -- against torch.float64 on the device, PER ELEMENT, each called directly through
its gemm.py entry point (the router is not involved).  Cases, input families (graded / cancel / exact), the reference and the bound:
tests/gemm_bf16_cases.py; the GELU terms of the bars: tests/golden/gemm_bf16_bars.json (measured on the CPU, never from a kernel).

    TN        every case at M = 1, 63, 65, 130 (the weight-stationary kernel also at 32 * 257 + 5: its ring wraps), with and without bias,
              on the three families: graded and cancel within the bound, exact bit-equal to fp64
    rows      rows [0, 33) computed alone == the same rows of the 130-row product, bit for bit (the fixed accumulation order)
    NT        splits 1 / default / 2, big tiles, the slab sum inside the launch, three problems of different shapes in one launch
    fence     every operand a window of a NaN buffer (two rows above and below, 8 columns on each side inside a pitch of K + 16, the
              bias at offset 4 of a NaN vector), the destination a window of a buffer of 7.0: finite, within the bound, bit-equal to
              the call on contiguous copies, sentinels untouched.  A kernel that stages a neighbouring value and multiplies it by
              zero fails here
    epilogues GELU forward (F to the TN bound, G to 1.13 bound_F + 2^-8 |g64| + m), GELU backward (dF with the bound propagated through
              the kernel's chain bf16(fl32(bf16(dg) * GELU'_fp32(fl32(f + b)))), the column partials' sum), pool (groups of 32 and 16:
              graded within the bound and equal to the max / first argmax of the kernel's own rows; exact -- full of ties -- bit-equal
              to the max over the group of the fp64 result, arg = the FIRST maximising row, as gm3d_group_max_fwd documents)

What this is for: tests/test_gpu_gemm.py compares two kernels with a library product under bars scaled by one global number and every
other kernel with those two; its inputs are randn.  An element off by 4e-3 where 5e-5 is allowed, a dropped last K-chunk, two swapped
output rows or a zeroed small row pass there (tests/test_gemm_bf16_cases_cpu.py) and fail here.

Measured (MI355X), worst error / bound over a kernel's cases (graded / cancel; every exact case bit-equal):
    linear_tn        0.990 / 0.991 (N = 256, K = 128 / the ragged N = 288, K = 96); fenced 0.987
    linear_tn_ring   0.990 / 0.985, the same at bm 64 and 128 (bit-identical); ring96 0.990 / 0.985; fenced 0.985
    linear_tn_dma    0.982 / 0.970; linear_tn_dmaw 0.986 / 0.958 at every bm x bn; fenced 0.978
    linear_tn_ws     0.993 / 0.983 (the 96-wide members); fenced 0.977
    wgrad_nt         0.023 / 0.012 in every form (R = 32, N = 576, K = 192), multi 0.023 / 0.012, fenced 0.023: fp32 results sit far
                     inside an any-order bound
    GELU forward     F 0.986, G 0.986; GELU backward dF 0.948, column sums 0.68; pool 0.991 (rows and pooled values)
The restatement on the CPU sits at 0.991: the kernels are at the one bf16 rounding they promise.  The NaN fences found nothing.
Found by the pool cases: gm3d_gemm_tn_bf16_pool (csrc/gemm.hip) with bias_after_pool and the rows wanted stored the rows WITH the bias
(9e6 x the bound on a graded element) where the other two carriers store the product that was pooled; fixed in csrc/gemm.hip.
"""
import functools

import pytest
import torch

from tests import gemm_bf16_cases as C

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def table():
    return C.bars()


@functools.lru_cache(maxsize=24)
def _problem(family, M, N, K):
    """x, w, b on the device and, without / with bias, (ref, bound) in fp64: computed once, shared, never modified"""
    x, w, b = (t.cuda() for t in C.tn_inputs(family, M, N, K))
    rb = []
    for bias in (None, b):
        ref, mag = C.tn_reference(x, w, bias)
        rb.append((ref, C.tn_bound(ref, mag, K)))
    return x, w, b, rb


def _fn(c):
    from gm3d_amd import gemm
    return functools.partial(getattr(gemm, c.kernel), **dict(c.args))


def _hold(what, got, ref, bound):
    """finite and within the bound -> worst error / bound"""
    assert bool(torch.isfinite(got).all()), (what, "non-finite")
    r = C.worst(got, ref, bound)
    if not r <= 1.0:
        pytest.fail("%s: %.3f x the bound, worst at %s" % (what, r, C.locate(got, ref, bound)))
    return r


@pytest.mark.parametrize("c", C.tn_cases(), ids=C.case_id)
def test_tn_against_fp64(c):
    fn, rows = _fn(c), C.rows_of(c)
    top = {}
    for family in C.FAMILIES:
        x, w, b, rb = _problem(family, rows[-1], c.N, c.K)
        for bias in (False, True):
            ref, bound = rb[bias]
            for M in rows:
                y = fn(x[:M], w, b if bias else None)
                assert tuple(y.shape) == (M, c.N) and y.dtype == torch.bfloat16
                what = "%s %s M=%d bias=%d" % (C.case_id(c), family, M, bias)
                if family == "exact":
                    assert torch.equal(y.double(), ref[:M]), (what, "not bit-equal to fp64", C.locate(y, ref[:M], bound[:M]))
                else:
                    top[family] = max(top.get(family, 0.0), _hold(what, y, ref[:M], bound[:M]))
    print("\nGEMM64 tn %s graded=%.3f cancel=%.3f" % (C.case_id(c), top["graded"], top["cancel"]))


@pytest.mark.parametrize("c", C.tn_cases(), ids=C.case_id)
def test_tn_rows_do_not_depend_on_m(c):
    fn, rows = _fn(c), C.rows_of(c)
    x, w, b, _ = _problem("graded", rows[-1], c.N, c.K)
    full = fn(x[:C.M_MAX], w, b)
    assert torch.equal(fn(x[:C.ROWS_ALONE], w, b), full[:C.ROWS_ALONE])
    assert torch.equal(fn(x[:C.M_MAX], w, b), full)
    if rows[-1] > C.M_MAX:
        assert torch.equal(fn(x, w, b)[:C.M_MAX], full)


def _window(t, fill, above=2, left=8):
    """-> (buffer, view): t as a window of a larger buffer of `fill`: `above` rows above and below, `left` columns on each side"""
    shape = tuple(t.shape[:-2]) + (t.shape[-2] + 2 * above, t.shape[-1] + 2 * left)
    buf = torch.full(shape, fill, dtype=t.dtype, device=t.device)
    view = buf[..., above:above + t.shape[-2], left:left + t.shape[-1]]
    view.copy_(t)
    return buf, view


def _untouched(buf, view, fill):
    """every element of `buf` outside `view` still holds `fill`"""
    saved = view.clone()
    view.fill_(fill)
    ok = bool((buf == fill).all())
    view.copy_(saved)
    return ok


@pytest.mark.parametrize("c", C.fence_cases(), ids=C.case_id)
def test_tn_nan_fence(c):
    from gm3d_amd import gemm
    fn, M = _fn(c), 65
    x, w, b, rb = _problem("graded", C.rows_of(c)[-1], c.N, c.K)
    x = x[:M]
    ref, bound = rb[1][0][:M], rb[1][1][:M]
    _, xv = _window(x, NAN)
    _, wv = _window(w, NAN)
    bb = torch.full((c.N + 8,), NAN, device="cuda")
    bv = bb[4:4 + c.N]
    bv.copy_(b)
    assert gemm._rows_ok(xv, 8) and gemm._rows_ok(wv, 8) and xv.stride(0) == c.K + 16 and wv.stride(0) == c.K + 16
    dst, dv = _window(torch.empty(M, c.N, dtype=torch.bfloat16, device="cuda"), 7.0)
    fn(xv, wv, bv, out=dv)
    r = _hold(C.case_id(c) + " fenced", dv, ref, bound)
    assert torch.equal(dv, fn(x, w, b)), (C.case_id(c), "differs from the call on contiguous copies")
    assert _untouched(dst, dv, 7.0), (C.case_id(c), "stored outside the destination window")
    print("\nGEMM64 fence %s %.3f" % (C.case_id(c), r))


# --------------------------------------------------------------------------------------------------------------------------------- NT

def _nt_run(c, dy, x, variant, out=None):
    from gm3d_amd import gemm
    _, splits, big, fuse = variant
    was = gemm.FUSE_SLAB_SUM
    gemm.FUSE_SLAB_SUM = fuse
    try:
        return gemm.wgrad_nt(dy, x, out, splits=splits, big_tiles=big)
    finally:
        gemm.FUSE_SLAB_SUM = was


@pytest.mark.parametrize("c", C.nt_cases(), ids=C.nt_case_id)
def test_nt_against_fp64(c):
    from gm3d_amd import gemm
    d = gemm.lib.gm3d_gemm_nt_splits(c.nb, c.R, c.N, c.K)
    top = {}
    for family in C.FAMILIES:
        dy, x = (t.cuda() for t in C.nt_inputs(family, c))
        assert gemm.wgrad_supported(dy, x)
        ref, mag = C.nt_reference(dy, x)
        for v in C.nt_variants(c, d):
            got = _nt_run(c, dy, x, v)
            assert tuple(got.shape) == (c.nb, c.N, c.K) and got.dtype == torch.float32
            what = "%s %s %s" % (C.nt_case_id(c), family, v[0])
            if family == "exact":
                assert torch.equal(got.double(), ref), (what, "not bit-equal to fp64")
            else:
                top[family] = max(top.get(family, 0.0), _hold(what, got, ref, C.nt_bound(mag, c.R, v[1] or d)))
    print("\nGEMM64 nt %s graded=%.3f cancel=%.3f" % (C.nt_case_id(c), top["graded"], top["cancel"]))


def test_nt_multi_against_fp64():
    from gm3d_amd import gemm
    top = {}
    for family in C.FAMILIES:
        ops = [tuple(t.cuda() for t in C.nt_inputs(family, c)) for c in C.NT_MULTI]
        assert all(gemm.wgrad_multi_ok(dy, x, None) for dy, x in ops)
        outs, spl = gemm.wgrad_nt_multi([(dy, x, None) for dy, x in ops], want_splits=True)
        for c, (dy, x), got, s in zip(C.NT_MULTI, ops, outs, spl):
            ref, mag = C.nt_reference(dy, x)
            if family == "exact":
                assert torch.equal(got.double(), ref), (c, "not bit-equal to fp64")
            else:
                top[family] = max(top.get(family, 0.0), _hold("multi %s %s" % (C.nt_case_id(c), family), got, ref, C.nt_bound(mag, c.R, s)))
    print("\nGEMM64 nt multi graded=%.3f cancel=%.3f" % (top["graded"], top["cancel"]))


@pytest.mark.parametrize("c", [C.NTCase(2, 1024, 128, 384), C.NTCase(2, 1024, 576, 192)], ids=C.nt_case_id)
def test_nt_nan_fence(c):
    """the widest fence wgrad_supported admits is the TN one: two rows above and below every batch, 8 columns on each side"""
    from gm3d_amd import gemm
    dy, x = (t.cuda() for t in C.nt_inputs("graded", c))
    ref, mag = C.nt_reference(dy, x)
    _, dyv = _window(dy, NAN)
    _, xv = _window(x, NAN)
    assert gemm.wgrad_supported(dyv, xv) and dyv.stride(1) == c.N + 16 and xv.stride(1) == c.K + 16
    d = gemm.lib.gm3d_gemm_nt_splits(c.nb, c.R, c.N, c.K)
    for v in C.nt_variants(c, d):
        dst, ov = _window(torch.empty(c.nb, c.N, c.K, device="cuda"), 7.0, above=2, left=4)
        _nt_run(c, dyv, xv, v, out=ov)
        r = _hold("%s %s fenced" % (C.nt_case_id(c), v[0]), ov, ref, C.nt_bound(mag, c.R, v[1] or d))
        assert torch.equal(ov, _nt_run(c, dy, x, v)), (c, v[0], "differs from the call on contiguous copies")
        assert _untouched(dst, ov, 7.0), (c, v[0], "stored outside the destination window")
        print("\nGEMM64 fence nt %s %s %.3f" % (C.nt_case_id(c), v[0], r))


def test_nt_multi_nan_fence():
    from gm3d_amd import gemm
    reqs, flats, plain = [], [], []
    for c in C.NT_MULTI:
        dy, x = (t.cuda() for t in C.nt_inputs("graded", c))
        _, dyv = _window(dy, NAN)
        _, xv = _window(x, NAN)
        stride = c.N * c.K + 256
        flat = torch.full((c.nb * stride + 64,), 7.0, device="cuda")
        out = torch.as_strided(flat, (c.nb, c.N, c.K), (stride, c.K, 1), 64)
        assert gemm.wgrad_multi_ok(dyv, xv, out)
        reqs.append((dyv, xv, out))
        flats.append((flat, torch.as_strided(flat, (c.nb, c.N * c.K), (stride, 1), 64)))
        plain.append((dy, x, None))
    outs, spl = gemm.wgrad_nt_multi(reqs, want_splits=True)
    want = gemm.wgrad_nt_multi(plain, splits=spl)
    for c, (dy, x, _), got, w_, s, (flat, view) in zip(C.NT_MULTI, plain, outs, want, spl, flats):
        ref, mag = C.nt_reference(dy, x)
        r = _hold("multi %s fenced" % C.nt_case_id(c), got, ref, C.nt_bound(mag, c.R, s))
        assert torch.equal(got, w_) and _untouched(flat, view, 7.0), c
        print("\nGEMM64 fence nt multi %s %.3f" % (C.nt_case_id(c), r))


# -------------------------------------------------------------------------------------------------------------------------- epilogues

@pytest.mark.parametrize("M", C.EPI_M)
@pytest.mark.parametrize("c", C.GELU_CASES, ids=C.case_id)
def test_gelu_forward_against_fp64(c, M, table):
    fn = _fn(c)
    x, w, b = (t.cuda() for t in C.tn_inputs("graded", M, c.N, c.K))
    ref_f, mag = C.tn_reference(x, w)
    bound_f = C.tn_bound(ref_f, mag, c.K)
    f, g = fn(x, w, b, f_out=torch.full((M, c.N), NAN, dtype=torch.bfloat16, device="cuda"))
    rf = _hold(C.case_id(c) + " F", f, ref_f, bound_f)
    g64, bound_g = C.gelu_bound(ref_f, bound_f, b, table["%s-M%d" % (C.case_id(c), M)]["c_gelu"])
    rg = _hold(C.case_id(c) + " G", g, g64, bound_g)
    assert torch.equal(fn(x, w, b)[1], g)                       # without F: the same G
    print("\nGEMM64 gelu %s M=%d F=%.3f G=%.3f" % (C.case_id(c), M, rf, rg))


@pytest.mark.parametrize("M", C.EPI_M)
@pytest.mark.parametrize("c", C.GELU_BWD_CASES, ids=C.case_id)
def test_gelu_backward_against_fp64(c, M, table):
    """The kernel's chain: dg = the fp32 product, rounded to bf16 like a stored GEMM result; gg = GELU'(fl32(f + b)) in fp32;
    v = fl32(bf16(dg) * gg); dF = bf16(v); the column partials add the fp32 v.  dF is held to the bound gemm_bf16_cases.gelu_bwd_bound
    propagates through that chain.  The partials' sum is compared with the fp64 column sum of dg64 * GELU'64: gamma(M) times the sum
    of magnitudes for the M adds, plus the elements' own bounds before the bf16 rounding (the partials add fp32 values that no output
    shows, so an fp64 reference carries every element's error with it)."""
    from gm3d_amd import gemm
    d_o, w2t, f, b = (t.cuda() for t in C.gelu_bwd_inputs(M, c.N, c.K))
    ref_dg, mag = C.tn_reference(d_o, w2t)
    mg = 3.0 * table["%s-M%d" % (C.case_id(c), M)]["d_gelu_grad"]
    df64, pre, bound = C.gelu_bwd_bound(ref_dg, C.tn_bound(ref_dg, mag, c.K), f, b, mg)
    tiles = gemm.tile_rows(M) if c.kernel == "linear_gelu_bwd" else -(-M // dict(c.args)["bm"])
    df = torch.full((M, c.N), NAN, dtype=torch.bfloat16, device="cuda")
    part = torch.full((tiles, c.N), NAN, device="cuda")
    _fn(c)(d_o, w2t, f, b, df, part)
    rd = _hold(C.case_id(c) + " dF", df, df64, bound)
    col_bound = C.gamma(M) * (df64.abs() + pre).sum(0) + pre.sum(0)
    rc = _hold(C.case_id(c) + " column sums", part.double().sum(0), df64.sum(0), col_bound)
    print("\nGEMM64 gelu_bwd %s M=%d dF=%.3f colsum=%.3f" % (C.case_id(c), M, rd, rc))


def _first_argmax(v):
    """v (G,k,N) -> (max (G,N), the first maximising row (G,N) uint8)"""
    top = v.max(1).values
    idx = torch.arange(v.shape[1], device=v.device)[None, :, None].expand_as(v)
    return top, torch.where(v == top[:, None], idx, v.shape[1]).min(1).values.to(torch.uint8)


@pytest.mark.parametrize("after", [False, True], ids=["bias-first", "bias-after"])
@pytest.mark.parametrize("c", C.pool_cases(), ids=C.pool_case_id)
def test_pool_against_fp64(c, after):
    from gm3d_amd import gemm
    top = 0.0
    for groups in C.POOL_GROUPS[c.group_rows]:
        M = groups * c.group_rows
        for family in ("graded", "exact"):
            x, w, b = (t.cuda() for t in C.tn_inputs(family, M, c.N, c.K, salt=11))
            route = (c.route, dict(c.args))
            rows, pooled, arg = gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=True, group_rows=c.group_rows, route=route)
            _, pooled2, arg2 = gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=False, group_rows=c.group_rows, route=route)
            assert torch.equal(pooled, pooled2) and torch.equal(arg, arg2)
            ref, mag = C.tn_reference(x, w, None if after else b)
            bound = C.tn_bound(ref, mag, c.K)
            ref_top, ref_arg = _first_argmax(ref.view(groups, c.group_rows, c.N))
            what = "%s %s groups=%d" % (C.pool_case_id(c), family, groups)
            if family == "exact":
                assert torch.equal(rows.double(), ref), (what, "rows not bit-equal to fp64")
                assert torch.equal(pooled.double(), ref_top + b.double() if after else ref_top), (what, "pooled")
                assert torch.equal(arg, ref_arg), (what, "arg is not the first maximising row")
                continue
            top = max(top, _hold(what + " rows", rows, ref, bound))
            own_top, own_arg = _first_argmax(rows.float().view(groups, c.group_rows, c.N))
            assert torch.equal(pooled, (own_top + b).bfloat16() if after else own_top.bfloat16()), (what, "pooled != max of the kernel's own rows")
            assert torch.equal(arg, own_arg), (what, "arg is not the first maximising row of the kernel's own rows")
            e = bound.view(groups, c.group_rows, c.N).max(1).values           # |max got - max ref| <= max of the elements' bounds
            if after:
                a = e + C.U * (ref_top.abs() + b.double().abs() + e)          # ... one fp32 add of the bias, one more bf16 rounding
                top = max(top, _hold(what + " pooled", pooled, ref_top + b.double(), a + C.HALF_ULP * ((ref_top + b.double()).abs() + a)))
            else:
                top = max(top, _hold(what + " pooled", pooled, ref_top, e))
    print("\nGEMM64 pool %s %s %.3f" % (C.pool_case_id(c), "after" if after else "first", top))

"""CPU: the cases and the bound of tests/test_gpu_gemm_bf16_fp64.py (tests/gemm_bf16_cases.py).  The restatement bf16(fp32 matmul + b)
is within the bound in every case and bit-equal to fp64 in the `exact` ones; the check rejects faults planted in the restatement that
the bars of tests/test_gpu_gemm.py miss; the case list covers every kernel and tile form and is checked against gemm.py; the GELU terms
of the committed table regenerate.  A TN case is checked on its M_MAX = 130 rows: the smaller M are row prefixes of the same problem and
the bound is per element (the wrap length of the weight-stationary kernel is a matter of the GPU test alone)."""
import importlib.util
import inspect
import os

import pytest
import torch

from tests import gemm_bf16_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problems():
    """the distinct (N, K) of the TN cases: the kernel and its arguments do not enter the inputs"""
    return sorted({(c.N, c.K) for c in C.tn_cases()})


@pytest.fixture(scope="module")
def graded():
    """(N, K) -> x, w, b and, with and without bias, (ref, bound) of the graded family at M_MAX rows: computed once"""
    out = {}
    for N, K in _problems():
        x, w, b = C.tn_inputs("graded", C.M_MAX, N, K)
        out[N, K] = (x, w, b, {bias: (lambda r, m: (r, C.tn_bound(r, m, K)))(*C.tn_reference(x, w, b if bias else None))
                               for bias in (False, True)})
    return out


def test_restatement_is_within_the_bound_and_exact_cases_are_bit_equal():
    top = {f: 0.0 for f in C.FAMILIES}
    for N, K in _problems():
        for family in C.FAMILIES:
            x, w, b = C.tn_inputs(family, C.M_MAX, N, K)
            assert x.dtype == w.dtype == torch.bfloat16 and b.dtype == torch.float32
            assert float(x.float().abs().max()) < 2.0 ** 40 and float(w.float().abs().max()) < 2.0 ** 40
            for bias in (None, b):
                ref, mag = C.tn_reference(x, w, bias)
                got = C.tn_restate(x, w, bias)
                if family == "exact":
                    assert float(mag.max()) <= 256.0, (N, K)                       # the precondition of bit-equality
                    assert torch.equal(got.double(), ref), (N, K)
                    assert K <= C.EXACT_NNZ or int((w != 0).sum(1).max()) == C.EXACT_NNZ
                else:
                    r = C.worst(got, ref, C.tn_bound(ref, mag, K))
                    top[family] = max(top[family], r)
                    assert r <= 1.0, (family, N, K, r, C.locate(got, ref, C.tn_bound(ref, mag, K)))
                if family == "cancel":
                    zero, _ = C.tn_reference(x, w)
                    assert float(zero.abs().max()) == 0.0                          # the true product is exactly zero
    print("restatement / bound: graded %.3f, cancel %.3f" % (top["graded"], top["cancel"]))
    assert 0.75 <= top["graded"] <= 1.0                                            # the bound is tight
    x, w, _ = C.tn_inputs("exact", C.M_MAX, 8, 8)
    assert bool(((w != 0).sum(0) == 1).all()) and bool(((w != 0).sum(1) == 1).all())   # one case multiplies by a column permutation


def test_graded_outputs_span_many_orders_of_magnitude(graded):
    x, w, b, rb = graded[256, 384]
    ref = rb[True][0].abs()
    assert float(ref.max() / ref.median()) > 2.0 ** 12 and float(ref.median() / ref[ref > 0].min()) > 2.0 ** 12
    rows = x.float().abs().amax(1)
    assert float(rows.max() / rows.min()) > 2.0 ** 20


def test_nt_restatement_is_within_the_bound_and_exact_cases_are_bit_equal():
    for c in list(C.nt_cases()) + list(C.NT_MULTI):
        for family in C.FAMILIES:
            dy, x = C.nt_inputs(family, c)
            ref, mag = C.nt_reference(dy, x)
            got = C.nt_restate(dy, x)
            if family == "exact":
                assert float(mag.max()) <= 2.0 ** 24
                assert torch.equal(got.double(), ref), c
            else:
                assert C.worst(got, ref, C.nt_bound(mag, c.R, 1)) <= 1.0, (family, c)
            if family == "cancel":
                assert float(ref.abs().max()) == 0.0


@pytest.mark.parametrize("fault", C.FAULTS)
def test_planted_faults_are_rejected_in_every_graded_case(fault, graded):
    """Measured: every fault is rejected in every graded case it applies to -- bias_late also in the K = 1536 cases, which are not
    required (the double rounding costs up to 2^-8 |F| against a bound whose accumulation term grows with K: on the graded inputs
    the worst element is at 4.45 .. 5.38 x the bound at K = 512, 2.10 at 1024, 1.65 at 1152 and 1.14 / 1.22 / 1.16 at K = 1536 with
    N = 128 / 256 / 384; an emulation on randn / sqrt(K) operands at M = 33, N = 384, K = 1536 gave 1.27)."""
    applied = 0
    for (N, K), (x, w, b, rb) in graded.items():
        for bias in (False, True):
            y = C.plant(fault, x, w, b if bias else None)
            if y is None:
                continue
            applied += 1
            ref, bound = rb[bias]
            r = C.worst(y, ref, bound)
            if fault == "bias_late" and K > C.BIAS_LATE_K:
                print("bias_late N=%d K=%d: %.2f x the bound (not required)" % (N, K, r))
                continue
            assert r > 1.0, (fault, N, K, bias, r)
    assert applied >= len(graded)


def _todays_test_gemm_tn_accepts(y, x, w, b):
    """the three assertions of tests/test_gpu_gemm.py::test_gemm_tn, as they stand"""
    ref = x.float() @ w.float().t() + b
    err = (y.float() - ref).abs()
    return (float((err / (ref.abs() + 1.0)).max()) <= 6e-3 and float(err.mean()) <= 3e-3 * float(ref.abs().mean())
            and (torch.equal(y, ref.bfloat16()) or float((y.float() - ref.bfloat16().float()).abs().max()) <= 2.0 ** -6 * float(ref.abs().max())))


def test_todays_bar_accepts_a_small_element_moved_by_4e_3():
    """test_gemm_tn's inputs (randn, W / sqrt(K); its (100, 64, 128) case): the restatement with one element of |ref| < 2^-8 moved by
    4e-3 passes all three of its assertions and is 75 x and more over the per-element bound."""
    M, K, N = 100, 64, 128
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g)
    ref, mag = C.tn_reference(x, w, b)
    bound = C.tn_bound(ref, mag, K)
    good = C.tn_restate(x, w, b)
    assert C.worst(good, ref, bound) <= 1.0 and _todays_test_gemm_tn_accepts(good, x, w, b)
    bad = C.plant("move_small", x, w, b)
    assert int((bad != good).sum()) == 1
    assert _todays_test_gemm_tn_accepts(bad, x, w, b)
    assert C.worst(bad, ref, bound) > 50.0


def test_case_list_covers_every_kernel_and_tile_form_of_gemm_py():
    from gm3d_amd import gemm
    from gm3d_amd._capi import lib
    cs = C.tn_cases()
    assert len({C.case_id(c) for c in cs}) == len(cs)
    kernels = {c.kernel for c in cs} | {c.kernel for c in C.GELU_CASES + C.GELU_BWD_CASES}
    # every bf16 product entry point of gemm.py that launches ONE kernel of the family (the LayerNorm, residual and BatchNorm forms are
    # covered elsewhere: tests/test_gpu_fused_ln.py, tests/test_gpu_gemm.py)
    entry = {n for n, f in inspect.getmembers(gemm, inspect.isfunction) if n.startswith(("linear_tn", "linear_gelu")) and not n.endswith("_f32")}
    assert kernels == entry, (kernels, entry)
    for c in list(cs) + list(C.GELU_CASES + C.GELU_BWD_CASES):
        params = inspect.signature(getattr(gemm, c.kernel)).parameters
        assert all(k in params for k, _ in c.args), c
    for n in ("linear_pool", "wgrad_nt", "wgrad_nt_multi", "route_pool", "wgrad_supported", "wgrad_multi_ok", "tile_rows"):
        assert callable(getattr(gemm, n))
    assert {"splits", "big_tiles"} <= set(inspect.signature(gemm.wgrad_nt).parameters) and hasattr(gemm, "FUSE_SLAB_SUM")
    assert C.OWN_KT == gemm.OWN_KT

    def of(kernel):
        return [c for c in cs if c.kernel == kernel]

    own = of("linear_tn")
    assert {c.K // 64 for c in own if c.N % 128 == 0 and c.K % 64 == 0} == set(gemm.OWN_KT) | {3, 5}
    assert {(c.K, c.N) for c in own if c.N % 128 or c.K % 64} == {(8, 8), (40, 72), (96, 288), (288, 96), (72, 136)}
    for bm in (64, 128):
        ring = [c for c in of("linear_tn_ring") if dict(c.args)["bm"] == bm]
        assert {(c.K, c.N) for c in ring if c.N % 128 == 0} == {(K, N) for K in (128, 384, 1536) for N in (128, 384)}
        assert {c.N for c in ring if c.N % 128} == {8, 96, 136, 200}
        assert {c.N for c in of("linear_tn_ring96") if dict(c.args)["bm"] == bm} == {96, 192, 384}
        assert {c.N for c in of("linear_tn_dma") if dict(c.args)["bm"] == bm} == {192, 1152}
        assert {dict(c.args)["bn"] for c in of("linear_tn_dmaw") if dict(c.args)["bm"] == bm} == {128, 192, 256}
    assert all(c.N % dict(c.args)["bn"] == 0 for c in of("linear_tn_dmaw"))
    admitted = {(N, K) for N in range(8, 1025, 8) for K in range(8, 1025, 8) if lib.gm3d_gemm_ws_supported(N, K, 0)}
    assert {(c.N, c.K) for c in of("linear_tn_ws")} == admitted == set(C.WS_NK)
    assert {(N, K) for N in range(8, 1025, 8) for K in range(8, 1025, 8) if lib.gm3d_gemm_ws_supported(N, K, 1)} == set(C.WS_POOL_NK)
    assert C.rows_of(of("linear_tn_ws")[0])[-1] == 32 * 257 + 5 and C.TN_M == (1, 63, 65, 130) and C.ROWS_ALONE == 33
    assert {(c.kernel, c.args) for c in C.fence_cases()} == {(c.kernel, c.args) for c in cs}      # the NaN fence reaches every tile form
    assert set(C.fence_cases()) <= set(cs)
    pools = C.pool_cases()
    assert {p.route for p in pools} == {"own", "dma", "ws", "ws16"} and {p.group_rows for p in pools} == {16, 32}
    assert {(p.N, p.K) for p in pools if p.route in ("ws", "ws16")} == set(C.WS_POOL_NK)


def test_nt_cases_follow_the_contract():
    from gm3d_amd._capi import lib
    cs = C.nt_cases()
    assert {(c.N, c.K) for c in cs} == {(8, 8), (96, 96), (128, 384), (576, 192)}
    assert min(c.R for c in cs) == 32 and all(c.R % 32 == 0 for c in cs)          # R % 32 == 0 is the contract: no ragged last stage exists
    for c in cs:
        d = lib.gm3d_gemm_nt_splits(c.nb, c.R, c.N, c.K)
        assert d == (2 if c.R == 1024 else 1), c                                  # one R gives 2 slabs by default
        names = [v[0] for v in C.nt_variants(c, d)]
        assert names[:2] == ["splits1", "default"] and ("splits2" in names) == (c.R % 64 == 0)
        assert ("big1" in names) == ((c.N, c.K) == (128, 384)) and ("sum2" in names) == (c.R % 64 == 0)
    assert len(C.NT_MULTI) == 3 and len({(c.nb, c.R, c.N, c.K) for c in C.NT_MULTI}) == 3 and all(c.K % 4 == 0 for c in C.NT_MULTI)


def test_gelu_terms_regenerate():
    """the committed GELU terms are what the recipe gives here, to a quarter (another libm's erf may differ in the last bits; a
    figure taken from a kernel would not be this recipe's) -- and of the size an fp32 erf explains"""
    spec = importlib.util.spec_from_file_location("make_gemm_bf16_bars", os.path.join(ROOT, "tests", "golden", "make_gemm_bf16_bars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    now, committed = mod.generate(), C.bars()
    assert sorted(now) == sorted(committed)
    assert sorted(committed) == sorted("%s-M%d" % (C.case_id(c), M) for c in C.GELU_CASES + C.GELU_BWD_CASES for M in C.EPI_M)
    for k, row in committed.items():
        assert row == pytest.approx(now[k], rel=0.25), k
        assert 0.0 < row.get("c_gelu", 1.0) < 16.0 and 0.0 < row.get("d_gelu_grad", 1e-7) < 1e-6, k

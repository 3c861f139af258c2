"""-m gpu: every op family of the Python layer, forward and backward, with every `empty` allocation poisoned (tests/poison.py).

Each case builds its inputs once, runs the operation plain twice (is it bitwise repeatable?), then once under NaN, +inf and -inf: the
poisoned results must equal the plain one bit for bit (the one operation that does not repeat itself bitwise, an atomic scatter, is named
in AT_A_BAR and held to its own test's bar).  A difference means a kernel read an element nobody wrote -- a partial row a
block skipped, a pad column of a ragged tile, a host-side row count one larger than the grid, a `0 * C + acc` epilogue, a max-pool over
pad rows.  The shapes are the smallest that still reach the ragged tiles, empty blocks, split / slab paths and dead rows of each
kernel, not the workload's.  The last test is the coverage condition over the allocation sites of gm3d_amd/."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import clouds, poison
from tests.poison import assert_same, assert_within, leaves, poisoned

pytestmark = pytest.mark.gpu
PATTERNS = ["nan", "+inf", "-inf"]
DTYPES = [torch.float32, torch.bfloat16]
DT = {torch.float32: "f32", torch.bfloat16: "bf16"}
CASES = {}           # id -> factory() -> (run, options); run() -> nested tensors
RAN = set()
# Cases whose two PLAIN runs differ bitwise (an atomic scatter): the tensors named here are compared at the bar their own existing test
# holds them to (a fraction of the tensor's largest entry) and may not turn non-finite; every other tensor of the case stays bitwise.
# The tensors are named, not detected: two plain runs can agree by chance where the third, poisoned one does not.
# {id: (bar, leaves, why)}.  Nothing else may be listed here.
AT_A_BAR = {
    "chamfer-P5-n50-m70": (1e-5, ("[4]", "[5]"),
                           "both input gradients: the general Chamfer backward (every shape but the 8- and 16-point patches) adds each pair's "
                           "term to both clouds' gradients with float atomics (csrc/chamfer.hip chamfer_bwd_general_kernel); with more than "
                           "one wave per cloud (70 points) the order of the additions varies from launch to launch.  Bar of "
                           "tests/test_gpu_kernels.py::test_chamfer_forward_backward"),
}


def case(name):
    def deco(factory):
        assert name not in CASES, name
        CASES[name] = factory
        return factory
    return deco


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=g) * scale).cuda().to(dtype)


def grads(*ts):
    return [None if t is None else t.grad for t in ts]


def leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _leaf_bitwise(x, y):
    if not isinstance(x, torch.Tensor):
        return x == y
    if not x.dtype.is_floating_point:
        return torch.equal(x, y)
    xn, yn = x.isnan(), y.isnan()
    return torch.equal(xn, yn) and torch.equal(x.masked_fill(xn, 0), y.masked_fill(yn, 0))


# ------------------------------------------------------------------------------------------------------------------ sampling / grouping
for _N, _G in [(100, 17), (300, 300), (1025, 64)]:
    @case("fps-N%d-G%d" % (_N, _G))
    def _(N=_N, G=_G):
        from gm3d_amd import ops
        x = clouds.gaussian(3, N, seed=N + G).cuda()
        return lambda: (ops.fps(x, G), ops.furthest_point_sample(x, G))

for _N, _G, _k in [(100, 7, 64), (64, 3, 64), (1025, 5, 32)]:
    @case("knn-N%d-G%d-k%d" % (_N, _G, _k))
    def _(N=_N, G=_G, k=_k):
        from gm3d_amd import ops
        x = clouds.uniform(3, N, seed=N + k).cuda()
        q = x[:, torch.randperm(N, generator=gen(G))[:G]].contiguous()

        def run():
            dist, idx = ops.knn(x, q, k)
            d2, i2 = ops.KNN(k, transpose_mode=True)(x, q)
            return dist, idx, d2, i2, ops.knn(x, q, k, return_dist=False)[1]
        # every query is a point of the cloud: its nearest neighbour is itself at distance 0, the other columns are not
        return run

    @case("knn_group-N%d-G%d-k%d" % (_N, _G, _k))
    def _(N=_N, G=_G, k=_k):
        from gm3d_amd import ops
        x = clouds.gaussian(2, N, seed=N + 3 * k).cuda()
        _, c = ops.fps(x, G)
        return lambda: (ops.knn_group(x, c, k), ops.knn_group(x, c, k, return_idx=False, return_org=False)[0])


@case("gather_operation")
def _():
    from gm3d_amd import ops
    g = gen(5)
    f = randn(g, 3, 7, 100)
    idx = torch.randint(0, 100, (3, 33), generator=g).int().cuda()
    idx[:, 5] = idx[:, 4]          # a repeated source column: its gradient is a sum
    w = randn(g, 3, 7, 33)

    def run():
        fi = leaf(f)
        out = ops.gather_operation(fi, idx)
        (out * w).sum().backward()
        return out, fi.grad
    return run


# ------------------------------------------------------------------------------------------------------------------ Chamfer
for _P, _n, _m in [(7, 32, 32), (5, 50, 70), (3, 1, 9), (37, 8, 8), (41, 16, 16)]:
    @case("chamfer-P%d-n%d-m%d" % (_P, _n, _m))
    def _(P=_P, n=_n, m=_m):
        from gm3d_amd import ops
        g = gen(P * 131 + n)
        a = torch.rand(P, n, 3, generator=g) - 0.5
        b = torch.rand(P, m, 3, generator=g) - 0.5
        if n == m:                     # exact duplicates across the two clouds and inside one cloud: argmin ties
            b[:, :3] = a[:, :3]
            a[:, 5 % n] = a[:, 4 % n]
        a, b = a.cuda(), b.cuda()
        g1, g2 = randn(g, P, n), randn(g, P, m)

        def run():
            ai, bi = leaf(a), leaf(b)
            d1, d2, i1, i2 = ops.chamfer(ai, bi)
            ((d1 * g1).sum() + (d2 * g2).sum()).backward()
            with torch.no_grad():
                mods = (ops.ChamferDistanceL2(reduction="mean")(a, b), ops.ChamferDistanceL1()(a, b))
            return d1, d2, i1, i2, ai.grad, bi.grad, mods
        return run

for _dt in DTYPES:
    for _B, _M in [(3, 1), (4, 39)]:
        for _full in (False, True):
            @case("patch_chamfer-%s-B%d-M%d%s" % (DT[_dt], _B, _M, "-full" if _full else ""))
            def _(dt=_dt, B=_B, M=_M, full=_full):
                from gm3d_amd import heads
                L = 64
                g = gen(B * 7 + M)
                pix = randn(g, B, L, 96, scale=0.3, dtype=dt)
                target = randn(g, B, L, 32, 3, scale=0.3)
                order = torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).cuda()
                mask_ids = order[:, L - M:]

                def run():
                    p = leaf(pix)
                    pred = p if full else p[:, L - M:]
                    assert heads.patch_chamfer_loss_supported(p[:, L - M:], target, mask_ids)
                    mean, matrix = heads.PatchChamferLossFn.apply(pred, target, mask_ids, full)
                    i1, i2 = mean.grad_fn.saved_tensors[3:5]
                    (mean * 3.0).backward()
                    return mean, matrix, i1, i2, p.grad
                return run

    for _B, _Mn in [(1, 1), (2, 38)]:
        @case("patch_chamfer_l1-%s-B%d-M%d" % (DT[_dt], _B, _Mn))
        def _(dt=_dt, B=_B, Mn=_Mn):
            from gm3d_amd import heads
            L = 64
            g = gen(B * 7 + Mn)
            pix = randn(g, B, L, 96, scale=0.3, dtype=dt)
            target = randn(g, B, L, 32, 3, scale=0.3)
            order = torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).cuda()
            mask_ids = order[:, L - Mn:]

            def run():
                p = leaf(pix)
                mean, matrix = heads.PatchChamferL1LossFn.apply(p[:, L - Mn:], target, mask_ids)
                i1, i2 = mean.grad_fn.saved_tensors[3:5]
                (mean * 3.0).backward()
                return mean, matrix, i1, i2, p.grad
            return run


# ------------------------------------------------------------------------------------------------------------------ attention
for _dt in DTYPES:
    for _T in [1, 25, 65, 129, 257]:
        @case("attention-%s-T%d" % (DT[_dt], _T))
        def _(dt=_dt, T=_T):
            from gm3d_amd import ops
            B, H = 3, 6
            g = gen(T)
            qkv = randn(g, B, T, 3 * H * 64, scale=1.5, dtype=dt)
            w = randn(g, B, T, H * 64, dtype=dt)
            backward = not (dt == torch.bfloat16 and T > 256)      # the bf16 backward's contract ends at 256 tokens

            def run():
                q = leaf(qkv)
                out = ops.attention(q, H, 0.125)
                if not backward:
                    return out.detach(), None
                (out.float() * w.float()).sum().backward()
                return out, q.grad
            return run

    for _T, _hd in [(13, 64), (33, 16), (200, 32)]:
        @case("attention_masked-%s-T%d-hd%d" % (DT[_dt], _T, _hd))
        def _(dt=_dt, T=_T, hd=_hd):
            from gm3d_amd import ops
            B, H = 3, 6
            g = gen(T + hd)
            c = torch.rand(B, T, 3, generator=g)
            m = torch.cdist(c, c) >= 0.9
            n = torch.randint(max(T // 2, 1), T, (B,), generator=g)           # n < T: every cloud has padded (dead) queries
            valid = torch.arange(T).unsqueeze(0) < n.unsqueeze(1)
            mask = (m | ~valid.unsqueeze(1) | ~valid.unsqueeze(2)).cuda()
            assert bool(mask.all(dim=2).any())
            bits = ops.pack_mask(mask)
            qkv = randn(g, B, T, 3 * H * hd, scale=1.2, dtype=dt)
            w = randn(g, B, T, H * hd, dtype=dt)

            def run():
                q = leaf(qkv)
                out = ops.attention_masked(q, bits, H, hd ** -0.5)
                (out.float() * w.float()).sum().backward()
                return out, q.grad               # the dead queries' rows are zeros by definition; the others are not
            return run


for _B, _T in [(1, 1), (2, 33)]:
    @case("attention_qkv_fused-B%d-T%d" % (_B, _T))
    def _(B=_B, T=_T):
        from gm3d_amd import attention
        H = 6                        # the fused qkv + attention forward: bf16, C = 384, T <= 64
        g = gen(33 + T)
        h = randn(g, B * T, 384, dtype=torch.bfloat16)
        wqkv = randn(g, 1152, 384, scale=0.05, dtype=torch.bfloat16)
        assert attention.qkv_supported(h, wqkv, T, H)
        return lambda: (attention.qkv_fwd(h, wqkv, B, T, H, 0.125, want_qkv=True, want_lse=True),
                        attention.qkv_fwd(h, wqkv, B, T, H, 0.125)[0])


# ------------------------------------------------------------------------------------------------------------------ row operations
for _dt in DTYPES:
    for _R, _T in [(3, 1), (200, 25)]:
        @case("residual_ln-%s-R%d-T%d" % (DT[_dt], _R, _T))
        def _(adt=_dt, R=_R, T=_T):
            from gm3d_amd import fused
            g = gen(R)
            res, y, add = randn(g, R, 384), randn(g, R, 384, dtype=adt), randn(g, R, 384, dtype=adt)
            bias, gamma, beta = randn(g, 384, scale=0.3), 1 + randn(g, 384, scale=0.2), randn(g, 384, scale=0.1)
            rs = ((torch.rand(R // T, generator=g) > 0.3).float() / 0.7).cuda()
            rs[0] = 1 / 0.7
            dh, gin = randn(g, R, 384, dtype=adt), randn(g, R, 384)

            def run():
                out_res, h, mean, rstd = fused.residual_ln_fwd(res, y, bias, rs, T, add, gamma, beta, 1e-5, adt, R)
                o2, h2, _, _ = fused.residual_ln_fwd(res, None, None, None, 1, None, gamma, beta, 1e-5, adt, R)
                acc = torch.ones(R, 384, device="cuda")
                dx, dy, sums = fused.residual_ln_bwd(dh, gin, out_res, mean, rstd, gamma, rs, T, acc, True, adt, R)
                return out_res, h, mean, rstd, o2, h2, acc, dx, dy, sums
            return run

    for _C in (100, 384):
        for _R in (7, 4100):
            for _form in ["plain", "xz", "xy", "xybias_scale", "all"]:
                @case("add_layer_norm-%s-%s-C%d-R%d" % (_form, DT[_dt], _C, _R))
                def _(adt=_dt, C=_C, R=_R, form=_form):
                    from gm3d_amd import heads
                    B = 7 if R == 7 else 4          # R = B * T rows
                    T = R // B
                    g = gen(C + len(form) + R)
                    x = randn(g, B, T, C, dtype=adt)
                    y = randn(g, B, T, C, dtype=adt) if form in ("xy", "xybias_scale", "all") else None
                    z = randn(g, B, T, C, dtype=adt) if form in ("xz", "all") else None
                    yb = randn(g, C, scale=0.5) if form in ("xybias_scale", "all") else None
                    rs = None
                    if form in ("xybias_scale", "all"):
                        rs = ((torch.rand(B, generator=g) > 0.3).float() / 0.7).cuda()
                        rs[0] = 1 / 0.7
                    w, b = 1 + randn(g, C, scale=0.2), randn(g, C, scale=0.2)
                    gs, gh = randn(g, B, T, C, dtype=adt), randn(g, B, T, C, dtype=adt)

                    def run():
                        xi, yi, zi, ybi, wi, bi = leaf(x), leaf(y), leaf(z), leaf(yb), leaf(w), leaf(b)
                        s, h = heads.AddLayerNormFn.apply(xi, yi, ybi, rs, zi, wi, bi, 1e-5, adt)
                        (s.float() * gs.float()).sum().add((h.float() * gh.float()).sum()).backward()
                        return s, h, grads(xi, yi, zi, ybi, wi, bi)
                    return run

    @case("layer_norm-%s-C4-R1" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import heads
        g = gen(1004)
        x = (randn(g, 1, 4, scale=1.5) + 0.3).to(dt)
        w, b, dy = (torch.rand(4, generator=g) + 0.5).cuda(), randn(g, 4, scale=0.2), randn(g, 1, 4, dtype=dt)

        def run():
            xi, wi, bi = leaf(x), leaf(w), leaf(b)
            h = heads.LayerNormFn.apply(xi, wi, bi, 1e-5, dt)
            h.backward(dy)
            return h, grads(xi, wi, bi)
        return run

    for _R, _C in [(7, 128), (200, 1536)]:
        @case("bias_gelu-%s-R%d-C%d" % (DT[_dt], _R, _C))
        def _(adt=_dt, R=_R, C=_C):
            from gm3d_amd import fused, heads
            g = gen(R + C)
            f, bias, dg = randn(g, R, C, scale=2, dtype=adt), randn(g, C, scale=0.5), randn(g, R, C, dtype=adt)

            def run():
                out = fused.bias_gelu_fwd(f, bias, adt)
                df, db = fused.bias_gelu_bwd(dg, f, bias, adt)
                fi, bi = leaf(f), leaf(bias)
                o2 = heads.BiasGeluFn.apply(fi, bi, adt)
                o2.backward(dg)
                return out, df, db, o2, fi.grad, bi.grad
            return run

    for _R, _C in [(300, 2048), (4096, 24)]:
        @case("colsum-%s-R%d-C%d" % (DT[_dt], _R, _C))
        def _(adt=_dt, R=_R, C=_C):
            from gm3d_amd import embed
            m = randn(gen(R + C), R, C, dtype=adt)
            return lambda: embed.colsum(m, adt)


# ------------------------------------------------------------------------------------------------------------------ GEMM
class _switch:
    """a module switch set for the length of a run (the switches are module attributes, not environment variables)"""

    def __init__(self, mod, **kw):
        self.mod, self.kw = mod, kw

    def __enter__(self):
        self.was = {k: getattr(self.mod, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.mod, k, v)

    def __exit__(self, *exc):
        for k, v in self.was.items():
            setattr(self.mod, k, v)


# one case per name gemm.route returns: the smallest M and width tests/golden/gemm_routes.json lists for it, and the table's ragged M
# (200: no multiple of a 64-row tile) where it has one.  (M, N, K), operand type, F32_OWN
ROUTES = [("ring", 64, 96, 384, torch.bfloat16, False), ("ring", 200, 96, 384, torch.bfloat16, False),
          ("dmaw", 64, 256, 128, torch.bfloat16, False), ("dmaw", 200, 256, 128, torch.bfloat16, False),
          ("own", 64, 8, 8, torch.bfloat16, False), ("own", 200, 8, 8, torch.bfloat16, False),
          ("ws", 32768, 96, 288, torch.bfloat16, False),
          ("f32", 200, 96, 384, torch.float32, True), ("lib", 200, 96, 384, torch.float32, False)]
for _kind, _M, _N, _K, _dt, _own in ROUTES:
    @case("mm-%s-M%d-N%d-K%d" % (_kind, _M, _N, _K))
    def _(kind=_kind, M=_M, N=_N, K=_K, dt=_dt, own=_own):
        from gm3d_amd import gemm
        g = gen(M + N + K)
        x, w, b = randn(g, M, K, dtype=dt), randn(g, N, K, scale=K ** -0.5, dtype=dt), randn(g, N)
        d = randn(g, M, N, dtype=dt)

        def run():
            with _switch(gemm, F32_OWN=own):
                assert gemm.route(x, w)[0] == kind
                out = torch.empty(M, N, dtype=dt, device="cuda")          # the caller's own destination: written whole, too
                gemm.mm(x, w, b, out=out)
                return gemm.mm(x, w), gemm.mm(x, w, b), out, gemm.mm_nn(d, w)      # and the layer's input gradient d @ w
        return run, {"foreign_allocations": kind == "lib"}


for _M in (77, 200):
    @case("linear_gelu-M%d" % _M)
    def _(M=_M):
        from gm3d_amd import gemm
        g = gen(M)
        C, Hd = 384, 1536
        x, w1, b1 = randn(g, M, C, dtype=torch.bfloat16), randn(g, Hd, C, scale=C ** -0.5, dtype=torch.bfloat16), randn(g, Hd, scale=0.3)
        d_o, w2t = randn(g, M, C, dtype=torch.bfloat16), randn(g, Hd, C, scale=Hd ** -0.5, dtype=torch.bfloat16)

        def run():
            f = torch.empty(M, Hd, dtype=torch.bfloat16, device="cuda")
            _, gl = gemm.linear_gelu(x, w1, b1, f_out=f)
            g2 = gemm.linear_gelu(x, w1, b1)[1]
            fd, gd = gemm.linear_gelu_dma(x, w1, b1, f_out=torch.empty_like(f))
            df = torch.empty(M, Hd, dtype=torch.bfloat16, device="cuda")
            colpart = torch.empty(gemm.tile_rows(M), Hd, dtype=torch.float32, device="cuda")
            gemm.linear_gelu_bwd(d_o, w2t, f, b1, df, colpart)
            df2 = torch.empty_like(df)
            cp2 = torch.empty(-(-M // 64), Hd, dtype=torch.float32, device="cuda")
            gemm.linear_gelu_bwd_dma(d_o, w2t, f, b1, df2, cp2, bm=64)
            outs = [f, gl, g2, fd, gd, df, colpart.sum(0), df2, cp2.sum(0)]
            # the same products through the dispatcher: what route_gelu / route_gelu_bwd name for each stack (tiled: TransformerStackFn's
            # rule) and under the switches that send them to the tiled and the split forms
            for tiled, sw in [(True, {}), (True, {"USE_DMA": False}), (False, {}), (False, {"USE_DMA": False})]:
                with _switch(gemm, **sw):
                    outs.append(gemm.mm_gelu(x, w1, b1, True, tiled=tiled))
                    outs.append(gemm.mm_gelu(x, w1, b1, False, tiled=tiled)[1])
                    route = gemm.route_gelu_bwd(d_o, w2t.t(), tiled=tiled)
                    cp = torch.empty(route[2], Hd, dtype=torch.float32, device="cuda")
                    outs += [gemm.mm_gelu_bwd(d_o, w2t, f, b1, torch.empty_like(df), cp, route), cp.sum(0)]
            assert [gemm.route_gelu(x, w1, tiled=t)[0] for t in (True, False)] == ["dma", "dma"]
            return outs
        return run


# (groups, group rows, K, N, bias after the pool, rows wanted): the register-prefetch / LDS-DMA pool kernels below 32768 rows, the
# weight-stationary ones (32- and 16-row groups) from there on, each with an odd number of groups (a last tile that is not full)
for _groups, _gr, _K, _N, _after, _rows in [(37, 32, 128, 256, False, True), (37, 32, 512, 384, True, False), (1025, 32, 128, 256, False, True),
                                            (1025, 32, 512, 384, True, False), (2051, 16, 512, 96, True, False),
                                            (2049, 16, 128, 256, False, True)]:
    @case("linear_pool-g%d-k%d-K%d-N%d" % (_groups, _gr, _K, _N))
    def _(groups=_groups, gr=_gr, K=_K, N=_N, after=_after, rows=_rows):
        from gm3d_amd import gemm
        M = groups * gr
        g = gen(groups + K)
        x = randn(g, M, K, dtype=torch.bfloat16)
        x[gr:2 * gr] = x[0:gr]
        x[5] = x[3]
        w, b = randn(g, N, K, scale=K ** -0.5, dtype=torch.bfloat16), randn(g, N, scale=0.2)

        def run():
            outs = [gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=rows, group_rows=gr)]
            route = gemm.route_pool(x, w, gr)
            assert route[0] == ("ws16" if gr == 16 else "ws" if M >= 32768 else "dma")
            outs.append(gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=rows, group_rows=gr, route=route))
            if gr == 32 and M < 32768:
                with _switch(gemm, POOL_ON_DMA=False):
                    outs.append(gemm.linear_pool(x, w, b, bias_after_pool=after, want_rows=rows))
            return outs
        return run

for _groups, _gr in [(1031, 32), (2062, 16)]:
    @case("ws_bn-g%d-k%d" % (_groups, _gr))
    def _(groups=_groups, gr=_gr):
        from gm3d_amd import gemm
        M, K, N = groups * gr, 256, 512
        g = gen(groups)
        x, w = randn(g, M, K, dtype=torch.bfloat16), randn(g, N, K, scale=K ** -0.5, dtype=torch.bfloat16)
        t, scale, shift = randn(g, groups, N, dtype=torch.bfloat16), randn(g, N), randn(g, N, scale=0.3)
        assert gemm.ws_bn_supported(x, w, t, group_rows=gr)

        def run():
            got = gemm.linear_ws_bn_apply(x, w, t, scale, shift, group_rows=gr)
            prod, part = gemm.linear_ws_bn_stats(x, w, t, group_rows=gr)
            return got, prod, part, part.sum(0)
        return run


@case("wgrad-nt")
def _():
    from gm3d_amd import gemm
    g = gen(1)
    dy, x = randn(g, 3, 96, 128, dtype=torch.bfloat16), randn(g, 3, 96, 136, dtype=torch.bfloat16)
    assert gemm.wgrad_supported(dy, x) and gemm.lib.gm3d_gemm_nt_splits(3, 96, 128, 136) == 1
    return lambda: (gemm.wgrad(dy, x), gemm.wgrad(dy[0], x[0]))


@case("wgrad-nt-row-split")
def _():
    from gm3d_amd import gemm
    g = gen(2)
    dy, x = randn(g, 1, 8192, 96, dtype=torch.bfloat16), randn(g, 1, 8192, 288, dtype=torch.bfloat16)
    assert gemm.lib.gm3d_gemm_nt_splits(1, 8192, 96, 288) > 1
    pitched = torch.zeros(1, 96, 288 + 8, device="cuda")
    bdy, bx = randn(g, 2, 128, 128, dtype=torch.bfloat16), randn(g, 2, 128, 384, dtype=torch.bfloat16)      # one 128 x 384 tile

    def run():
        out = gemm.wgrad_nt(dy, x, pitched[:, :, :288])          # a pitched destination: the slabs are added by torch
        with _switch(gemm, FUSE_SLAB_SUM=True):
            fused_sum = gemm.wgrad_nt(dy, x, splits=4)
        return gemm.wgrad(dy, x), gemm.wgrad(dy[0], x[0]), out.clone(), fused_sum, gemm.wgrad_nt(bdy, bx, splits=4, big_tiles=True)
    return run


@case("wgrad-f32-own-slabs")
def _():
    from gm3d_amd import gemm
    g = gen(3)
    dy, x = randn(g, 8192, 96), randn(g, 8192, 384)
    assert gemm.nt_f32_splits(1, 8192, 96, 384) > 1

    def run():
        with _switch(gemm, F32_OWN=True):
            return gemm.wgrad(dy, x), gemm.wgrad(dy.view(2, 4096, 96), x.view(2, 4096, 384)), gemm.wgrad(dy[:64], x[:64])
    return run


@case("wgrad-pad-to-128")
def _():
    from gm3d_amd import gemm
    g = gen(4)
    dy, x = randn(g, 256, 96, dtype=torch.bfloat16), randn(g, 256, 384, dtype=torch.bfloat16)
    odd = (randn(g, 48, 96, dtype=torch.bfloat16), randn(g, 48, 384, dtype=torch.bfloat16))     # 48 rows: no multiple of the 32-row stage

    def run():
        with _switch(gemm, RAGGED=False):       # without the ragged widths the 96-wide layer is zero-padded to one 128-column tile
            padded = gemm.wgrad(dy, x)
        return padded, gemm.wgrad(*odd)
    return run


@case("wgrad-lib-split-k")
def _():
    from gm3d_amd import gemm
    g = gen(5)
    dy, x = randn(g, 4096, 96), randn(g, 4096, 40)                 # fp32 without F32_OWN: the library, rows cut SPLITK ways
    dyb, xb = randn(g, 2, 4096, 128), randn(g, 2, 4096, 64)        # a stack's: WGRAD_ROW_SPLIT ways

    def run():
        outs = [gemm.wgrad(dy, x), gemm.wgrad(dyb, xb), gemm.wgrad(dyb, xb, out=torch.empty(2, 128, 64, device="cuda"))]
        with _switch(gemm, SUM_FEW_ROWS=False):
            outs += [gemm.wgrad(dy, x), gemm.wgrad(dyb, xb)]
        return outs
    return run


@case("wgrad-multi")
def _():
    from gm3d_amd import gemm
    g = gen(6)
    reqs = []
    for nb, R, N, K in ((1, 8192, 96, 288), (2, 2048, 128, 136), (1, 64, 8, 8)):
        reqs.append((randn(g, nb, R, N, dtype=torch.bfloat16), randn(g, nb, R, K, dtype=torch.bfloat16), None))
    assert all(gemm.wgrad_multi_ok(*r) for r in reqs)

    def run():
        outs, spl = gemm.wgrad_nt_multi(reqs, want_splits=True)
        assert max(spl) > 1 and min(spl) == 1
        return outs, gemm.wgrad_nt_multi(reqs, splits=[4, 2, 1])
    return run


@case("transposes")
def _():
    from gm3d_amd import gemm
    g = gen(7)
    nblk, shapes = 3, [(136, 72), (8, 264), (96, 96)]
    per = sum(a * b for a, b in shapes) + 640
    flat = randn(g, nblk * per, dtype=torch.bfloat16)
    groups, off = [], 0
    for a, b in shapes:
        groups.append([flat[i * per + off:i * per + off + a * b].view(a, b) for i in range(nblk)])
        off += a * b
    loose = [randn(g, 72, 40, dtype=torch.bfloat16) for _ in range(2)]
    return lambda: (gemm.stacked_transposes(groups), [gemm.stacked_transpose(ws) for ws in groups], gemm.transposed(groups[0][1]),
                    gemm.stacked_transpose(loose), gemm.stacked_transpose(groups[1][:1]))


# ------------------------------------------------------------------------------------------------------------------ mini-PointNet embed
def _bn_fill(m, running=True):
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm1d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
                if running:
                    mod.running_mean.uniform_(-0.2, 0.2)
                    mod.running_var.uniform_(0.5, 1.5)
    return m


def _embed_result(enc, tok, train, extra=()):
    res = {"tokens": tok.detach(), "buffers": {k: b.detach().clone() for k, b in enc.named_buffers()}, "extra": list(extra)}
    if train:
        res["grads"] = {k: p.grad.detach().clone() for k, p in enc.named_parameters()}
    return res


# a bias in front of a BatchNorm has a gradient of exactly zero: the embed returns zeros (layer 1) or the rounding residue of a sum of
# cancelling terms (layer 3) for it by definition
ZERO_BIAS = {"['first_conv.0.bias']": True, "['second_conv.0.bias']": True}

for _dt in DTYPES:
    for _B, _G, _V, _train in [(3, 16, None, True), (2, 64, None, True), (2, 64, None, False), (3, 16, 5, True), (4, 64, 25, True)]:
        @case("embed-%s-B%d-G%d%s%s" % (DT[_dt], _B, _G, "-V%d" % _V if _V else "", "" if _train else "-eval"))
        def _(dt=_dt, B=_B, G=_G, V=_V, train=_train):
            from gm3d_amd import models_mae_learn_loss as M
            torch.manual_seed(B * 100 + G)
            base = _bn_fill(M.Encoder(384).cuda())
            g = gen(B + G)
            nb = randn(g, B, G, 32, 3, scale=0.2)
            vis = None
            if V:
                order = torch.stack([torch.randperm(G, generator=g) for _ in range(B)]).cuda()
                vis = order[:, :V]
            w = randn(g, B, V or G, 384)

            def run():
                enc = copy.deepcopy(base).train(train)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                    if train:
                        tok = enc(nb, vis_ids=vis) if vis is not None else enc(nb)
                        (tok.float() * w).sum().backward()
                    else:
                        with torch.no_grad():
                            tok = enc(nb)
                return _embed_result(enc, tok, train)
            return run, {"exempt": ZERO_BIAS}

    @case("embed-m2ae-level0-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import embed, point_m2ae as P
        torch.manual_seed(5)
        base = _bn_fill(P.TokenEmbed(3, 96).cuda().train(), running=False)
        g = gen(50)
        nb, w = randn(g, 2, 512, 16, 3, scale=0.2), randn(g, 2, 512, 96)

        def run():
            enc = copy.deepcopy(base)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                tok = embed.run_embed(enc, nb)
                (tok.float() * w).sum().backward()
            return _embed_result(enc, tok, True)
        return run, {"exempt": ZERO_BIAS}

    @case("embed-m2ae-deep-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import point_m2ae as P
        torch.manual_seed(96 + 256)
        base = _bn_fill(P.TokenEmbed(96, 192).cuda().train(), running=False)
        g = gen(51)
        x, w = randn(g, 2, 256, 8, 96, scale=0.5), randn(g, 2, 256, 192)

        def run():
            enc = copy.deepcopy(base)
            xi = leaf(x)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                tok = enc._forward_fused(xi)
                (tok.float() * w).sum().backward()
            return _embed_result(enc, tok, True, extra=[xi.grad])
        return run, {"exempt": ZERO_BIAS}


# ------------------------------------------------------------------------------------------------------------------ heads and index ops
for _dt in DTYPES:
    for _train in (True, False):
        @case("heads-%s-%s" % (DT[_dt], "train" if _train else "eval"))
        def _(dt=_dt, train=_train):
            from gm3d_amd import heads
            from gm3d_amd import models_mae_learn_loss as M
            torch.manual_seed(3)
            base = M.mae_vit_base_patch16_dec512d8b()
            # the three heads and what they read: the positional MLP, the 96-wide reconstruction conv, the loss-prediction head,
            # the mask token
            with torch.no_grad():
                bn = base.increase_dim_2[1]
                bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3)
                bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
                base.mask_token.normal_()
            base = base.cuda()
            B, L = 2, 64
            g = gen(64)
            center = (torch.rand(B, L, 3, generator=g) - 0.5).cuda()
            xr, w_pos, w_pix, w_lp = randn(g, B, L, 384), randn(g, B, L, 384), randn(g, B, L, 96), randn(g, B, L)
            sd = {k: v.detach().clone() for k, v in base.state_dict().items() if "increase_dim_2" in k}

            def run():
                m = base.train(train)
                m.load_state_dict(sd, strict=False)                # the BatchNorm buffers move with every training forward
                m.zero_grad(set_to_none=True)
                x = xr.clone().requires_grad_(train)
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16), torch.set_grad_enabled(train):
                    pos = m.embed_pos(center)
                    c = m.increase_dim_just_network_without_feature[0]
                    pix = heads.LinearBiasFn.apply(x, c.weight, c.bias, heads._adt())
                    tok = heads.ExpandRowsFn.apply(m.mask_token, B, 5, pos.dtype)
                    lp = m._loss_pred_head(x)
                    if train:
                        ((pos.float() * w_pos).sum() + (pix.float() * w_pix).sum() + (lp.float() * w_lp).sum()
                         + (tok.float() * w_pos[:, :5]).sum()).backward()
                res = {"pos": pos.detach(), "pix": pix.detach(), "lp": lp.detach(),
                       "bn": {k: b.detach().clone() for k, b in m.increase_dim_2.named_buffers()}}
                if train:
                    res["grads"] = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
                    res["dx"] = x.grad
                return res
            # the conv in front of the head's BatchNorm: its bias has an exactly zero gradient, up to the rounding residue of the sum
            return run, {"exempt": {"['increase_dim_2.0.bias']": True}}

    for _B, _G in [(1, 7), (5, 64)]:
        @case("lin3_gelu-%s-B%d-G%d" % (DT[_dt], _B, _G))
        def _(dt=_dt, B=_B, G=_G):
            from gm3d_amd import heads
            g = gen(B + G)
            center = (torch.rand(B, G, 3, generator=g) - 0.5).cuda()
            w0, b0, w1, b1 = randn(g, 128, 3), randn(g, 128, scale=0.2), randn(g, 384, 128, scale=0.1), randn(g, 384, scale=0.2)
            w = randn(g, B, G, 384)

            def run():
                ps = [leaf(t) for t in (w0, b0, w1, b1)]
                out = heads.PosEmbedFn.apply(center, *ps, dt)
                (out.float() * w).sum().backward()
                return out, grads(*ps)
            return run

    for _V in (1, 25):
        @case("token_assemble-%s-V%d" % (DT[_dt], _V))
        def _(dt=_dt, V=_V):
            from gm3d_amd import heads
            from gm3d_amd import models_mae_learn_loss as M
            B, L, C = 7, 64, 384
            g = gen(V)
            mask = torch.zeros(B, L, dtype=torch.bool)
            for b in range(B):
                mask[b, torch.randperm(L, generator=g)[: L - V]] = True
            vis_ids, mask_ids = M.split_ids(mask.cuda(), V)
            tok, pos = randn(g, B, L, C, dtype=dt), randn(g, B, L, C, dtype=dt)
            w = [randn(g, B, V, C, dtype=dt), randn(g, B, V, C, dtype=dt), randn(g, B, L, C, dtype=dt)]

            def run():
                ti, pi = leaf(tok), leaf(pos)
                xv, pv, pf = heads.token_assemble(ti, pi, vis_ids, mask_ids)
                ((xv * w[0]).sum() + (pv * w[1]).sum() + (pf * w[2]).sum()).backward()
                p2 = leaf(pos)
                pv2, pf2 = heads.pos_assemble(p2, vis_ids, mask_ids, dt)
                ((pv2 * w[1]).sum() + (pf2 * w[2]).sum()).backward()
                return xv, pv, pf, ti.grad, pi.grad, pv2, pf2, p2.grad
            return run

    for _B, _S, _J, _C in [(1, 7, 40, 8), (5, 64, 768, 384)]:
        @case("take_rows-%s-B%d-S%d-J%d-C%d" % (DT[_dt], _B, _S, _J, _C))
        def _(dt=_dt, B=_B, S=_S, J=_J, C=_C):
            from gm3d_amd import heads
            g = gen(S + J)
            x, dy = randn(g, B, S, C, dtype=dt), randn(g, B, J, C, dtype=dt)
            ids = torch.randint(0, S - 1, (B, J), generator=g).cuda()          # row S-1 is never read: its gradient is zero

            def run():
                xi = leaf(x)
                y = heads.take_rows(xi, ids)
                y.backward(dy)
                return y, xi.grad
            return run

    @case("where_rows-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import heads
        B, T, C = 5, 77, 96
        g = gen(77)
        masked = (torch.rand(B, T, generator=g) < 0.6).cuda()
        a, alt, tok, w = randn(g, B, T, C, dtype=dt), randn(g, B, T, C, dtype=dt), randn(g, 1, 1, C), randn(g, B, T, C)

        def run():
            ai, li, ti = leaf(a), leaf(alt), leaf(tok)
            o1 = heads.where_rows(masked, ai, li)
            o2 = heads.where_rows(masked, ai, ti)
            ((o1.float() * w).sum() + (o2.float() * w).sum()).backward()
            return o1, o2, heads.where_rows(masked, a, None), grads(ai, li, ti)
        return run

    @case("interp3_group_max-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import heads
        B, N, S, C1, C2 = 3, 256, 64, 192, 384
        g = gen(2)
        fine, coarse = randn(g, B, N, C1, dtype=dt), randn(g, B, S, C2, dtype=dt)
        idx = torch.randint(0, S - 1, (B, N, 3), generator=g).cuda()          # coarse token S-1 has no reader
        w = torch.rand(B, N, 3, generator=g).cuda()
        w = w / w.sum(-1, keepdim=True)
        go = randn(g, B, N, C1 + C2)
        x = randn(g, 40, 8, 96, dtype=dt)
        x[3, 5] = x[3, 2]

        def run():
            fi, ci, xi = leaf(fine), leaf(coarse), leaf(x)
            out = heads.Interp3Fn.apply(fi, ci, idx, w)
            (out.float() * go).sum().backward()
            y = heads.GroupMaxFn.apply(xi)
            y.float().sum().backward()
            return out, y, grads(fi, ci, xi)
        return run


for _B, _L, _M in [(33, 40, 2), (7, 64, 64)]:
    @case("rank_loss-B%d-L%d-M%d" % (_B, _L, _M))
    def _(B=_B, L=_L, M=_M):
        from gm3d_amd import heads
        g = gen(B + M)
        full, target = randn(g, B, L), torch.rand(B, M, generator=g).cuda()
        if M > 6:
            target[:, 5] = target[:, 6]

        def run():
            fa, fb = leaf(full), leaf(full)
            a = heads.rank_loss_tail(fa, M, target)
            (a * 1.7).backward()
            b = heads.rank_loss(fb[:, -M:], target)
            (b * 1.7).backward()
            return a, fa.grad, b, fb.grad
        return run


@case("rank_loss-zero-over-zero")
def _():
    from gm3d_amd import heads
    g = gen(9)
    full, target = randn(g, 9, 39), torch.ones(9, 39).cuda()         # equal targets: no ranked pair, the loss is the documented 0 / 0

    def run():
        fa = leaf(full)
        return {"tail": heads.rank_loss_tail(fa, 39, target), "plain": heads.rank_loss(full, target)}
    return run, {"exempt": {"['tail']": True, "['plain']": True}}


for _B, _L, _ratio, _epoch in [(5, 64, 0.6, 0), (2, 64, 0.6, 200)]:
    @case("mask_select-B%d-epoch%d" % (_B, _epoch))
    def _(B=_B, L=_L, ratio=_ratio, epoch=_epoch):
        from gm3d_amd import models_mae_learn_loss as M
        g = gen(B * 1000 + L)
        lp, noise = torch.randn(B, L, generator=g), torch.rand(B, L, generator=g)
        if B == 2:                       # heavy ties
            lp, noise = (lp * 2).round() / 2, (noise * 8).floor() / 8
        lp, noise = lp.cuda(), noise.cuda()
        return lambda: (M.generate_mask_ids(lp, ratio, True, epoch, 400, noise),
                        M.generate_mask_ids(lp, ratio, True, epoch, 400, noise, want_bool=True))

for _B, _G, _nm in [(2, 65, 1), (3, 64, 38)]:
    @case("mask_centers-B%d-G%d-m%d" % (_B, _G, _nm))
    def _(B=_B, G=_G, nm=_nm):
        from gm3d_amd import heads
        g = gen(G + nm)
        noise = torch.rand(B, G, generator=g)
        noise[:, 7] = noise[:, 40]
        center = torch.randn(B, G, 3, generator=g)
        center[1, 11] = center[1, 4]
        start = torch.tensor([G - 1, 4, 0][:B], dtype=torch.int32).cuda()
        noise, center = noise.cuda(), center.cuda()
        return lambda: (heads.mask_centers(noise, nm), heads.mask_centers(center, nm, start=start))


@case("partition_visible-select_rows")
def _():
    from gm3d_amd import masked_stack as S
    g = gen(3)
    sets = []
    for B, T, Tc, p in ((7, 256, 96, 0.8), (3, 64, 16, 0.85), (2, 77, 77, 0.3)):
        masked = torch.rand(B, T, generator=g) < p
        for b in range(B):
            v = (~masked[b]).nonzero().flatten()
            if len(v) > Tc:
                masked[b, v[Tc:]] = True
        sets.append((masked.cuda(), Tc, randn(g, B, T, 96, dtype=torch.bfloat16), randn(g, B, T, 3),
                     randn(g, B, T, 96, dtype=torch.bfloat16)))
    flag = S.overflow_flag(torch.device("cuda"))
    crowded = torch.zeros(2, 64, dtype=torch.bool, device="cuda")

    def run():
        outs = []
        flag.zero_()
        for masked, Tc, x16, x3, tok in sets:
            part = S.partition_visible(masked, Tc)
            xc = S.select_rows(x16, part["perm_c"])
            outs.append((part, xc, S.select_rows(xc, part["inv_v"], tok), S.select_rows(xc, part["inv_v"]),
                         S.select_rows(x3, part["perm_c"])))
        assert int(flag) == 0
        over = S.partition_visible(crowded, 16)               # more visible tokens than the bound: reported, the lists still whole
        assert int(flag) == 1
        flag.zero_()
        return outs, over
    return run


@case("compact_merge")
def _():
    from gm3d_amd import masked_stack as S
    g = gen(1)
    B, T, Tc, C = 4, 256, 96, 192
    masked = (torch.rand(B, T, generator=g) < 0.75).cuda()
    x, tok, w = randn(g, B, T, C), randn(g, B, T, C), randn(g, B, T, C)

    def run():
        part = S.partition_visible(masked, Tc)
        xi, ti = leaf(x), leaf(tok)
        out = S.MergeFn.apply(S.CompactFn.apply(xi, part) * 2.0, ti, part)
        (out * w).sum().backward()
        return out, xi.grad, ti.grad
    return run


@case("back_project-radius_mask_bits")
def _():
    from gm3d_amd import ops
    from gm3d_amd import point_m2ae as P
    g = gen(0)
    B = 5
    idxs = [torch.randint(0, 2048, (B, 512, 16), generator=g).cuda(), torch.randint(0, 512, (B, 256, 8), generator=g).cuda(),
            torch.randint(0, 256, (B, 64, 8), generator=g).cuda()]
    coarse = (torch.rand(B, 64, generator=g) < 0.8).cuda()
    cen = clouds.pc_norm(torch.randn(B, 77, 3, generator=g)).cuda()
    vis = (torch.rand(B, 77, generator=g) < 0.7).cuda()
    return lambda: (P.back_project(coarse, idxs), ops.radius_mask_bits(cen, vis, 0.64), ops.radius_mask_bits(cen, None, 0.64),
                    ops.radius_mask_bits(cen, None, 0.64, masked=~vis))


@case("drop_path_scales-scale_translate")
def _():
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.engine_pretrain import PointcloudScaleAndTranslate
    aug = PointcloudScaleAndTranslate()
    pc = randn(gen(11), 7, 1024, 3)

    def run():
        torch.manual_seed(5)
        scales = M.drop_path_scales(34, [0.0, 0.003, 0.05, 0.1], True, torch.device("cuda"))
        drop = C.dropout_factors(3, (0.5, 0.5), torch.device("cuda"))
        moved = aug(pc.clone(), generator=torch.Generator(device="cuda").manual_seed(11))
        return [s for s in scales if s is not None], drop, moved
    return run


# ------------------------------------------------------------------------------------------------------------------ block stacks
def _seeded_drop_path(state):
    def scale(Bn, p, training, device):
        if p == 0.0 or not training:
            return None
        state[0] += 1
        m = ((1 - p) + torch.rand(Bn, generator=gen(100 + state[0]))).floor_()
        return (m / (1 - p)).to(device)
    return scale


for _dt in DTYPES:
    @case("fused_stack-%s-B4-T25-n3" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import models_mae_learn_loss as M
        torch.manual_seed(7)
        B, T = 4, 25
        dec = M.TransformerDecoder(embed_dim=384, depth=3, drop_path_rate=[0.0, 0.2, 0.3], num_heads=6).cuda().train()
        for p in dec.parameters():
            if p.dim() == 1:
                p.data.add_(0.1 * torch.randn_like(p))
        g = gen(25)
        x, pos, w = randn(g, B, T, 384), randn(g, B, T, 384), randn(g, B, T, 384)

        def run():
            xs, ps = leaf(x), leaf(pos)
            dec.zero_grad(set_to_none=True)
            with _switch(M, drop_path_scale=_seeded_drop_path([0]), FUSED_STACK=True):
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                    out = dec(xs, ps, 0)
                (out.float() * w).sum().backward()
            return out, xs.grad, ps.grad, {k: p.grad.clone() for k, p in dec.named_parameters()}
        return run

    @case("fused_stack-inference-%s-B32" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import models_mae_learn_loss as M
        torch.manual_seed(8)
        B, T = 32, 25                      # an inference-only stack from 32 clouds on runs as two parallel chains into ONE output buffer
        dec = M.TransformerDecoder(embed_dim=384, depth=2, drop_path_rate=[0.0, 0.1], num_heads=6).cuda().eval()
        g = gen(32)
        x, pos = randn(g, B, T, 384), randn(g, B, T, 384)

        def run():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
                return dec(x, pos, 0)
        return run

    for _B, _T, _C, _radius in [(4, 256, 192, 0.64), (8, 64, 384, 0.0)]:
        @case("masked_stack-%s-B%d-T%d-C%d" % (DT[_dt], _B, _T, _C))
        def _(dt=_dt, B=_B, T=_T, C=_C, radius=_radius):
            from gm3d_amd import models_mae_learn_loss as MM
            from gm3d_amd import ops
            from gm3d_amd import point_m2ae as P
            torch.manual_seed(0)
            stack = P.BlockStack(C, 3, 6, [0.0, 0.05, 0.1]).cuda().train()
            g = gen(T + C)
            x, pos = randn(g, B, T, C), randn(g, B, T, C, scale=0.3)
            cen = clouds.pc_norm(torch.randn(B, T, 3, generator=g)).cuda()
            vis = (torch.rand(B, T, generator=g) < 0.7).cuda()
            bits = ops.radius_mask_bits(cen, vis, radius) if radius > 0 else None
            keep = vis.unsqueeze(-1) if bits is not None else torch.ones(B, T, 1, dtype=torch.bool, device="cuda")
            lin = torch.linspace(0.5, 1.5, C, device="cuda")
            bf16 = dt == torch.bfloat16

            def run():
                xi, pi = leaf(x), leaf(pos)
                stack.zero_grad(set_to_none=True)
                with _switch(MM, drop_path_scale=_seeded_drop_path([0])):
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                        out = stack(xi.bfloat16() if bf16 else xi, pi.bfloat16() if bf16 else pi, bits)
                    # the rows of invisible tokens are not results of the stack (nothing reads them): selected away, not multiplied away
                    seen = torch.where(keep, out.float(), torch.zeros((), device="cuda"))
                    (seen * lin).sum().backward()
                return seen, xi.grad, pi.grad, {k: v.grad.detach().clone() for k, v in stack.named_parameters()}
            return run


# ------------------------------------------------------------------------------------------------------------------ tails and evaluation
def _tail_head(F_in, cls_dim, seed):
    torch.manual_seed(seed)
    h = nn.Sequential(nn.Linear(F_in, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
                      nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5), nn.Linear(256, cls_dim))
    with torch.no_grad():
        for bn in (h[1], h[5]):
            bn.weight.uniform_(0.8, 1.2)
            bn.bias.uniform_(-0.1, 0.1)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    return h.cuda()


for _dt in DTYPES:
    for _mode in (0, 1):
        for _train in (True, False):
            @case("cls_tail-%s-mode%d-%s" % (DT[_dt], _mode, "train" if _train else "eval"))
            def _(dt=_dt, mode=_mode, training=_train):
                from gm3d_amd import ops
                B, T, cls_dim = 5, 64, 40
                g = gen(mode)
                x0 = randn(g, B, T, 384, dtype=dt)
                x0[1, 7] = x0[1, 3]                     # an exact tie in the max-pool
                labels = torch.randint(0, cls_dim, (B,), generator=g).cuda()
                w = randn(g, B, cls_dim)
                drop = ((torch.rand(2, B, 256, generator=g) >= 0.5).float() / 0.5).cuda()
                base = _tail_head(384 * (2 if mode else 1), cls_dim, mode + 1)

                def run():
                    hk = copy.deepcopy(base).train(training)
                    xk = leaf(x0)
                    zk, lk = ops.cls_tail(xk, hk, mode, training, drop=drop, labels=labels)
                    res = {"logits": zk.detach(), "loss": lk.detach(),
                           "only_logits": ops.cls_tail(x0, copy.deepcopy(base).train(training), mode, training).detach()}
                    if training:
                        (lk + (zk * w).sum()).backward()
                        res["dx"] = xk.grad
                        res["grads"] = {k: p.grad.clone() for k, p in hk.named_parameters()}
                    res["buffers"] = {k: b.detach().clone() for k, b in hk.named_buffers()}
                    return res
                # the two Linear biases in front of a training-mode BatchNorm: a gradient of exactly zero by definition
                return run, {"exempt": {"['0.bias']": True, "['4.bias']": True}}

        @case("cls_tail_vote_pool-%s-mode%d" % (DT[_dt], _mode))
        def _(dt=_dt, mode=_mode):
            from gm3d_amd import ops
            V, B, T, cls_dim = 3, 5, 64, 15
            head = _tail_head(768 if mode else 384, cls_dim, 1000 + mode).eval()
            g = gen(V * B * T + mode)
            x = randn(g, V * B, T, 384, dtype=dt)
            labels = torch.randint(0, cls_dim, (B,), generator=g).cuda()

            def run():
                correct = torch.full((1,), 3, dtype=torch.long, device="cuda")
                votes = torch.empty(V, B, cls_dim, device="cuda")
                feat = torch.empty(V * B, 768 if mode else 384, device="cuda")
                mean, pred = ops.cls_tail_vote_pool(x, head, mode, labels, V, correct, votes=votes, feat=feat)
                m2, p2 = ops.cls_tail_vote_pool(x, head, mode, labels, V, correct)
                return mean, pred, votes, feat, m2, p2, correct
            return run

    @case("cls_tail_vote-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import ops
        V, B, T, cls_dim = 3, 5, 65, 15
        head = _tail_head(768, cls_dim, 65).eval()
        g = gen(T * cls_dim)
        x = randn(g, V * B, T, 384, dtype=dt)
        labels = torch.randint(0, cls_dim, (B,), generator=g).cuda()

        def run():
            correct = torch.full((1,), 5, dtype=torch.long, device="cuda")
            votes = torch.empty(V, B, cls_dim, device="cuda")
            mean, pred = ops.cls_tail_vote(x, head, labels, V, correct, votes=votes)
            m2, p2 = ops.cls_tail_vote(x, head, labels, V, correct)
            return mean, pred, votes, m2, p2, correct
        return run


@case("vote_sample")
def _():
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    B, N0, npoints, V = 3, 1100, 1024, 2
    pts = clouds.gaussian(B, N0, seed=B * 100 + V).cuda()
    point_all = EF.vote_point_all(npoints, N0)
    subsets, scale, shift = [torch.from_numpy(a).cuda() for a in EF.draw_votes(np.random.RandomState(V), point_all, npoints, V, B)]

    def run():
        fps_idx = ops.furthest_point_sample(pts, point_all)
        return fps_idx, ops.vote_sample(pts, fps_idx, subsets, scale, shift), EF.sample_points(pts, npoints, subset=subsets[0])
    return run


@case("svm")
def _():
    from gm3d_amd import svm
    from tests import svm_ref
    Xtr, ytr, Xte, yte = svm_ref.synthetic(300, 60, 4, 48, seed=5, sep=0.7)
    classes, inv = np.unique(ytr, return_inverse=True)
    order = np.argsort(inv, kind="stable")
    cs = np.concatenate([[0], np.cumsum(np.bincount(inv))]).tolist()
    Xg = torch.from_numpy(np.ascontiguousarray(Xtr[order])).cuda()
    Xt, yt = torch.from_numpy(Xte).cuda(), torch.from_numpy(np.searchsorted(classes, yte)).long().cuda()
    ytr_d = torch.from_numpy(ytr).cuda()

    def run():
        K = svm.gram(Xg)
        alpha, rho, iters, capped = svm.smo(K, cs, 0.01, 1e-3)
        w = svm.weights(Xg, cs, alpha)
        pred, correct = svm.vote(Xt, w, rho, len(cs) - 1, yt)
        clf = svm.LinearSVC().fit(torch.from_numpy(Xtr).cuda(), ytr_d)
        return (K, alpha, rho, iters, capped, w, pred, correct, svm.vote(Xt, w, rho, len(cs) - 1)[0], clf.coef_, clf.intercept_,
                clf.predict(Xt))
    return run


@case("knn_probe")
def _():
    from gm3d_amd import knn_probe as KP
    r = np.random.RandomState(305)
    ncls = 7
    # (300, 1, 64, 1) is the smallest case of the lattice tests; a second one with more rows than a block and k > 1
    sets = []
    for n, m, d, k in ((300, 1, 64, 1), (1027, 37, 64, 20)):
        X = (r.randn(n, d)).astype(np.float32)
        Q = (r.randn(m, d)).astype(np.float32)
        sets.append((torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda(), torch.from_numpy(r.randint(0, ncls, n)).long().cuda(),
                     torch.from_numpy(r.randint(0, ncls, m)).long().cuda(), k))

    def run():
        outs = []
        for X, Q, yx, yq, k in sets:
            Xn, Qn = KP.normalize(X), KP.normalize(Q)
            outs.append((Xn, Qn, KP.neighbours(Xn, Qn, k), KP.classify(Xn, yx, Qn, k, 0.07, ncls, test_labels=yq, return_probs=True),
                         KP.classify(Xn, yx, Qn, k, 0.07, ncls)[0], KP.knn_classifier(Xn, yx, Qn, yq, k, 0.07, ncls)))
        return outs
    return run


# ------------------------------------------------------------------------------------------------------------------ optimizer
for _lrd in (False, True):
    @case("flat_adamw_ema%s" % ("-lrd" if _lrd else ""))
    def _(lrd=_lrd):
        from gm3d_amd import engine_pretrain as E
        from gm3d_amd.optim import FlatAdamWEma
        g = gen(0)
        x = randn(g, 64, 37)

        def run():
            # the optimizer's own buffers are made with torch.zeros (its kernels accumulate into them); what is poisoned here is what
            # torch allocates for the model it flattens
            torch.manual_seed(0)
            net = nn.Sequential(nn.Linear(37, 53), nn.LayerNorm(53), nn.Linear(53, 11), nn.BatchNorm1d(11)).cuda()
            net.register_parameter("mask_token", nn.Parameter(torch.randn(1, 1, 7, device="cuda")))
            ema = E.ModelEma(net, decay=0.9)
            if lrd:
                opt = FlatAdamWEma(net, ema, lr=3e-3, weight_decay=0.05, max_norm=0.5,
                                   lr_scale_of=lambda n: 0.5 if n.startswith("0.") else 1.0)
            else:
                opt = E.build_optimizer(net, lr=3e-3, weight_decay=0.05, flat=True, model_ema=ema, clip_grad=0.5)
            norms = []
            for step in range(2):
                opt.zero_grad(set_to_none=True)
                (net(x * (1 + step)).pow(2).mean() * 50 + net.mask_token.sum()).backward()
                norms.append(E.step_update(net, ema, opt).clone())
            return norms, opt.P, opt.M, opt.V, opt.E, opt.PS, opt.ES, {k: b.clone() for k, b in net.named_buffers()}
        return run, {"foreign_allocations": True}


# ------------------------------------------------------------------------------------------------------------------ wrappers no model path calls bare
@case("weight_cache-pin")
def _():
    from gm3d_amd.fused import weight_cache
    torch.manual_seed(1)

    def run():
        m = nn.Sequential(nn.Linear(40, 24), nn.LayerNorm(24), nn.Linear(24, 8)).cuda()       # no flat optimizer: the cache owns the shadows
        torch.manual_seed(1)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=gen(p.numel())).cuda())
        weight_cache.pin(m)
        first = [weight_cache.get(p, torch.bfloat16).clone() for p in m.parameters() if p.dim() >= 2]
        with torch.no_grad():
            m[0].weight.mul_(2.0)
        weight_cache.refresh()
        return first, [weight_cache.get(p, torch.bfloat16).clone() for p in m.parameters() if p.dim() >= 2]
    return run


for _dt in DTYPES:
    @case("fused_attention_wrappers-%s" % DT[_dt])
    def _(dt=_dt):
        from gm3d_amd import attention
        B, T, H = 2, 25, 6
        g = gen(25)
        qkv, dout = randn(g, B * T, 3 * H * 64, scale=1.5, dtype=dt), randn(g, B * T, H * 64, dtype=dt)

        def run():
            out, lse = attention.fwd(qkv, None, B, T, H, 64, 0.125, head=True, pad=True)
            return out, lse, attention.bwd(qkv, None, out, dout, lse, B, T, H, 64, 0.125, head=True, pad=True)
        return run

    for _scaled in (True, False):
        @case("residual_tail-%s%s" % (DT[_dt], "-rowscale" if _scaled else ""))
        def _(dt=_dt, scaled=_scaled):
            from gm3d_amd import heads
            B, T, C = 6, 37, 96
            g = gen(37)
            x, y, yb, gs = randn(g, B, T, C, dtype=dt), randn(g, B, T, C, dtype=dt), randn(g, C, scale=0.5), randn(g, B, T, C, dtype=dt)
            rs = None
            if scaled:
                rs = ((torch.rand(B, generator=g) > 0.3).float() / 0.7).cuda()
                rs[0] = 1 / 0.7

            def run():
                xi, yi, bi = leaf(x), leaf(y), leaf(yb)
                s = heads.ResidualTailFn.apply(xi, yi, bi, rs, dt)
                (s.float() * gs.float()).sum().backward()
                return s, grads(xi, yi, bi)
            return run


@case("colsum_finish_f64")
def _():
    from gm3d_amd import heads
    part = torch.randn(5, 24, generator=gen(24), dtype=torch.float64).cuda()
    return lambda: heads._finish64(part, 5, 24)


@case("linear_bias_fn-96-wide")
def _():
    from gm3d_amd import gemm, heads
    g = gen(96)
    x, w, b, go = randn(g, 2, 128, 384), randn(g, 96, 384, 1, scale=0.05), randn(g, 96, scale=0.2), randn(g, 2, 128, 96)

    def run():
        outs = []
        for ragged in (True, False):        # without the ragged-width kernels the 96-wide gradient is zero-padded to one 128-column tile
            xi, wi, bi = leaf(x), leaf(w), leaf(b)
            with _switch(gemm, RAGGED=ragged):
                y = heads.LinearBiasFn.apply(xi, wi, bi, torch.bfloat16)
                (y.float() * go).sum().backward()
            outs.append((y, grads(xi, wi, bi)))
        return outs
    return run


def test_the_harness_catches_a_wrong_finish_on_the_device():
    """The CPU toys of tests/test_poison_cpu.py on device tensors: a finish that max-reduces a partial buffer with one unwritten row is
    caught under +inf and missed under nan; a correct one passes -- the patched allocators reach device memory."""
    x = (torch.rand(12, 6, generator=gen(0)) + 0.5).cuda()

    def finish(rows):
        part = torch.empty(rows, 6, device="cuda")
        for i in range(3):
            part[i] = x[i * 4:(i + 1) * 4].amax(0)
        best = part[0].clone()
        for i in range(1, rows):
            best = torch.where(part[i] > best, part[i], best)
        return best

    want = finish(3)
    seen = {}
    for pattern in PATTERNS:
        with poisoned(pattern) as ps:
            good, wrong = finish(3), finish(4)
        assert ps.count == 2 and ps.recorded == 0
        assert_same(want, good, "good")
        seen[pattern] = not torch.equal(want, wrong)
    assert seen == {"nan": False, "+inf": True, "-inf": False}


# ------------------------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("name", list(CASES))
def test_op_does_not_depend_on_unwritten_memory(name):
    made = CASES[name]()
    run, opt = made if isinstance(made, tuple) else (made, {})
    a = run()
    b = run()
    torch.cuda.synchronize()
    differ = [p for (p, x), (_, y) in zip(leaves(a), leaves(b)) if not _leaf_bitwise(x, y)]
    print("%s: plain vs plain %s" % (name, "bitwise equal" if not differ else "NOT bitwise equal at %s" % differ))
    loose = AT_A_BAR[name][1] if name in AT_A_BAR else ()
    assert set(differ) <= set(loose), "%s: two plain runs differ bitwise at %s, which is no documented atomic scatter" % (name, differ)
    for pattern in PATTERNS:
        ctx = poisoned(pattern)
        with ctx:
            got = run()
            torch.cuda.synchronize()
        ps = ctx.state
        print("%s / %s: %d poisoned allocations, %d from gm3d_amd/ at %s" % (name, pattern, ps.count, ps.recorded, sorted(ps.sites)))
        assert (ps.count if opt.get("foreign_allocations") else ps.recorded) >= 1, "no allocation was poisoned: a vacuous case"
        tag = "%s[%s]" % (name, pattern)
        la, lg = leaves(a), leaves(got)
        assert [p for p, _ in la] == [p for p, _ in lg], "%s: the two results differ in structure" % tag
        # every tensor that repeats bitwise must be bitwise under poison; the others (AT_A_BAR only) stay within their own test's bar
        assert_same({p: x for p, x in la if p not in loose}, {p: x for p, x in lg if p not in loose}, tag, exempt=opt.get("exempt"))
        if loose:
            assert_within({p: x for p, x in la if p in loose}, {p: x for p, x in lg if p in loose}, tag, AT_A_BAR[name][0])
    RAN.add(name)


EXPECTED = set(CASES)
poison.CASES[__name__] = (RAN, EXPECTED)


def test_every_allocation_site_is_reached_or_listed():
    """The coverage condition (tests/poison.py coverage): judged once this module ran whole; `every line reached or listed` over the
    union of both poison modules when both ran whole in this process (as the suite runs them), the list's own rules in any case."""
    if RAN != EXPECTED:
        pytest.skip("judged after the whole module ran (%d of %d cases did)" % (len(RAN), len(EXPECTED)))
    complete = all(ran == exp for ran, exp in poison.CASES.values()) and len(poison.CASES) == 2
    print("allocation sites: %d scanned, %d reached, %d listed (complete: %s)" % (poison.coverage(complete) + (complete,)))

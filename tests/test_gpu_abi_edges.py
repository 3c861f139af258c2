"""-m gpu: every kernel at the last shape its C-ABI guard accepts (tests/test_abi_limits_cpu.py holds the table), plus the shapes
where a launcher switches thread shape, kernel or LDS layout.  Each result is checked against a plain reference of the same
operation: the CPU oracle (FPS, KNN, Chamfer: bit-exact), torch index-op restatements (exact), fp64 torch (attention, GELU, the
classification head) at the bars of the existing tests.  Outputs written through raw pointers sit in front of a guard region
filled with a sentinel: the region must be untouched and no in-range element may keep the sentinel."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096        # elements of sentinel behind every guarded output


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


class Guarded:
    """A (shape) output in front of GUARD sentinel elements of the same dtype."""

    def __init__(self, shape, dtype, sentinel):
        n = math.prod(shape)
        self.buf = torch.full((n + GUARD,), sentinel, dtype=dtype, device="cuda")
        self.t = self.buf[:n].view(*shape)
        self.n, self.sentinel = n, sentinel

    def _is_sentinel(self, x):
        return torch.isnan(x) if isinstance(self.sentinel, float) and math.isnan(self.sentinel) else x == self.sentinel

    def check(self, name):
        torch.cuda.synchronize()
        assert bool(self._is_sentinel(self.buf[self.n:]).all()), "%s: write past the end" % name
        assert not bool(self._is_sentinel(self.t).any()), "%s: element left unwritten" % name
        return self.t


NAN = float("nan")
I32_SENT = -123456789


def _lib():
    from gm3d_amd._capi import lib
    return lib


def _ok(rc, what):
    from gm3d_amd._capi import check
    check(rc, what)


# ------------------------------------------------------------------ FPS: every thread-shape switch and the maximum N
@pytest.mark.parametrize("N", [256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384])
def test_fps_thread_shape_switches(oracle_ops, N):
    from gm3d_amd.ops import _ptr
    from tests import clouds
    B, npoint = 2, 96
    x = clouds.uniform(B, N, seed=N)
    want = oracle_ops.furthest_point_sample(x, npoint)
    xd = x.cuda()
    idx = Guarded((B, npoint), torch.int32, I32_SENT)
    cen = Guarded((B, npoint, 3), torch.float32, NAN)
    _ok(_lib().gm3d_fps(_ptr(xd), B, N, npoint, _ptr(idx.t), _ptr(cen.t), None), "fps")
    got = idx.check("fps idx").cpu()
    assert torch.equal(got, want)
    assert torch.equal(cen.check("fps centers").cpu(), torch.gather(x, 1, want.long().unsqueeze(-1).expand(-1, -1, 3)))


# ------------------------------------------------------------------ KNN: select / insertion switch at k = 64 and the maximum N
@pytest.mark.parametrize("N", [1024, 1025, 12288])
def test_knn_kernel_switch_and_max_n(oracle_ops, N):
    from gm3d_amd.ops import _ptr
    from tests import clouds
    B, G, k = 2, 64, 64
    x = clouds.uniform(B, N, seed=N + 1)
    q = x[:, torch.randperm(N, generator=torch.Generator().manual_seed(N))[:G]].contiguous()
    rd, ri = oracle_ops.knn(x, q, k)
    xd, qd = x.cuda(), q.cuda()
    dist = Guarded((B, G, k), torch.float32, NAN)
    idx = Guarded((B, G, k), torch.int64, -7)
    _ok(_lib().gm3d_knn(_ptr(xd), _ptr(qd), B, N, G, k, _ptr(dist.t), _ptr(idx.t), None), "knn")
    assert torch.equal(idx.check("knn idx").cpu(), ri)
    assert torch.equal(dist.check("knn dist").cpu(), rd)
    # the grouping form of the same kernel: neighbourhoods are exact fp32 differences of the gathered points
    idx2 = Guarded((B, G, k), torch.int64, -7)
    nb = Guarded((B, G, k, 3), torch.float32, NAN)
    nbo = Guarded((B, G, k, 3), torch.float32, NAN)
    _ok(_lib().gm3d_knn_group(_ptr(xd), _ptr(qd), B, N, G, k, _ptr(idx2.t), _ptr(nb.t), _ptr(nbo.t), None), "knn_group")
    assert torch.equal(idx2.check("knn_group idx").cpu(), ri)
    org = torch.gather(x, 1, ri.view(B, G * k, 1).expand(-1, -1, 3)).view(B, G, k, 3)
    assert torch.equal(nbo.check("knn_group org").cpu(), org)
    assert torch.equal(nb.check("knn_group nb").cpu(), org - q.unsqueeze(2))


# ------------------------------------------------------------------ Chamfer: the general kernel at grid.y = P = 65535
def test_chamfer_general_kernel_at_max_patches(oracle_ops):
    from gm3d_amd.ops import _ptr
    P, n, m = 65535, 20, 12
    g = torch.Generator().manual_seed(5)
    a = torch.rand(P, n, 3, generator=g) - 0.5
    b = torch.rand(P, m, 3, generator=g) - 0.5
    b[:, :2] = a[:, :2]                     # exact duplicates: argmin ties
    g1, g2 = torch.randn(P, n, generator=g), torch.randn(P, m, generator=g)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    d1r, d2r, i1r, i2r = oracle_ops.chamfer(ar, br)
    ((d1r * g1).sum() + (d2r * g2).sum()).backward()
    ad, bd, g1d, g2d = a.cuda(), b.cuda(), g1.cuda(), g2.cuda()
    d1, d2 = Guarded((P, n), torch.float32, NAN), Guarded((P, m), torch.float32, NAN)
    i1, i2 = Guarded((P, n), torch.int32, I32_SENT), Guarded((P, m), torch.int32, I32_SENT)
    _ok(_lib().gm3d_chamfer_fwd(_ptr(ad), _ptr(bd), P, n, m, _ptr(d1.t), _ptr(d2.t), _ptr(i1.t), _ptr(i2.t), None), "chamfer_fwd")
    assert torch.equal(d1.check("d1").cpu(), d1r.detach()) and torch.equal(d2.check("d2").cpu(), d2r.detach())
    assert torch.equal(i1.check("i1").cpu(), i1r) and torch.equal(i2.check("i2").cpu(), i2r)
    ga, gb = Guarded((P, n, 3), torch.float32, NAN), Guarded((P, m, 3), torch.float32, NAN)
    _ok(_lib().gm3d_chamfer_bwd(_ptr(ad), _ptr(bd), _ptr(i1.t), _ptr(i2.t), _ptr(g1d), _ptr(g2d), P, n, m, _ptr(ga.t), _ptr(gb.t),
                                None), "chamfer_bwd")
    for got, ref in ((ga.check("ga").cpu(), ar.grad), (gb.check("gb").cpu(), br.grad)):
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


# ------------------------------------------------------------------ attention: plain T = 128 | routed 129; masked T = 512 per head_dim
def _attention_ref(qkv, H, hd, bits_mask=None):
    B, T, _ = qkv.shape
    q64 = qkv.detach().double().requires_grad_(True)
    q, k, v = q64.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    if bits_mask is None:
        p = s.softmax(-1)
    else:
        none = bits_mask.all(-1, keepdim=True)[:, None]        # a query with no allowed key: zero output, zero gradients
        p = s.masked_fill(bits_mask[:, None], float("-inf")).masked_fill(none, 0.0).softmax(-1) * (~none)
    return q64, (p @ v).transpose(1, 2).reshape(B, T, H * hd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T", [128, 129])
def test_plain_attention_last_and_first_routed_length(dtype, T):
    from gm3d_amd import ops
    B, H, hd = 2, 6, 64
    g = torch.Generator(device="cuda").manual_seed(T)
    qkv = (torch.randn(B, T, 3 * H * hd, device="cuda", generator=g) * 0.7).to(dtype).requires_grad_(True)
    dout = torch.randn(B, T, H * hd, device="cuda", generator=g).to(dtype)
    out = ops.attention(qkv, H, hd ** -0.5)
    out.backward(dout)
    q64, ref = _attention_ref(qkv, H, hd)
    ref.backward(dout.double())
    tol_o, tol_g = (1e-5, 1e-5) if dtype == torch.float32 else (2e-2, 3e-2)
    assert rel(out, ref) <= tol_o and rel(qkv.grad, q64.grad) <= tol_g


@pytest.mark.parametrize("dtype,hd,T_fwd,T_bwd", [(torch.float32, 16, 512, 512), (torch.float32, 32, 512, 512),
                                                  (torch.float32, 64, 512, 512), (torch.bfloat16, 16, 512, 512),
                                                  (torch.bfloat16, 32, 512, 480), (torch.bfloat16, 64, 480, 256)])
def test_masked_attention_at_max_length(dtype, hd, T_fwd, T_bwd):
    """Forward at the longest accepted T, backward at the longest accepted T (bf16 keeps the head in LDS: head_dim 32 backward
    T <= 480, head_dim 64 T <= 480 / 256), with a
    radius mask that leaves some queries without any allowed key."""
    from gm3d_amd import ops
    from oracle import hier_ref as HR
    from tests import clouds
    B, H = 2, 3
    tol_o, tol_g = (1e-5, 1e-5) if dtype == torch.float32 else (2e-2, 3e-2)
    for T in sorted({T_fwd, T_bwd}):
        c = clouds.pc_norm(torch.randn(B, T, 3, generator=torch.Generator().manual_seed(T)))
        vis = torch.rand(B, T, generator=torch.Generator().manual_seed(T + 1)) < 0.8
        mask = ~(vis[:, :, None] & vis[:, None, :]) | HR.far_mask(c, 0.6)
        assert bool(mask.all(-1).any())                  # some queries have no allowed key
        bits = ops.pack_mask(mask.cuda())
        g = torch.Generator(device="cuda").manual_seed(T + hd)
        qkv = torch.randn(B, T, 3 * H * hd, device="cuda", generator=g).to(dtype).requires_grad_(True)
        dout = torch.randn(B, T, H * hd, device="cuda", generator=g).to(dtype)
        out = ops.attention_masked(qkv, bits, H, hd ** -0.5)
        q64, ref = _attention_ref(qkv, H, hd, mask.cuda())
        assert rel(out, ref) <= tol_o, (T, hd)
        if T == T_bwd:
            out.backward(dout)
            ref.backward(dout.double())
            assert rel(qkv.grad, q64.grad) <= tol_g, (T, hd)
    if dtype == torch.bfloat16 and T_bwd < 512:
        from gm3d_amd._capi import Gm3dError
        q = torch.zeros(1, T_bwd + 1, 3 * H * hd, device="cuda", dtype=dtype, requires_grad=True)
        with pytest.raises(Gm3dError):          # refused on the host: the head does not fit the LDS
            ops.attention_masked(q, None, H, 0.125).sum().backward()


# ------------------------------------------------------------------ radius mask bits: LDS above 64 KiB for G > 4096
def _packed_radius_mask(c, vis, radius, rows=512):
    """pack_mask(~(vis_i & vis_j) | far_mask) built row block by row block (the (B,G,G) mask at G = 8192 is large)."""
    B, G, _ = c.shape
    W = (G + 31) // 32
    weights = torch.ones(32, dtype=torch.int64, device=c.device) << torch.arange(32, device=c.device)
    out = torch.empty(B, G, W, dtype=torch.int32, device=c.device)
    r2 = torch.tensor(radius, dtype=torch.float32) * torch.tensor(radius, dtype=torch.float32)
    for i0 in range(0, G, rows):
        ci = c[:, i0:i0 + rows]
        d2 = None
        for ax in range(3):                              # hier_ref.far_mask's expression: every product and sum rounded to fp32
            diff = ci[:, :, None, ax] - c[:, None, :, ax]
            d2 = diff * diff if ax == 0 else d2 + diff * diff
        m = (d2 >= r2.to(c.device)) | ~(vis[:, i0:i0 + rows, None] & vis[:, None, :])
        full = torch.ones(B, m.shape[1], W * 32, dtype=torch.int64, device=c.device)
        full[:, :, :G] = m.to(torch.int64)
        words = (full.view(B, m.shape[1], W, 32) * weights).sum(-1)
        out[:, i0:i0 + rows] = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return out


@pytest.mark.parametrize("G", [4096, 4097, 8192])
def test_radius_mask_bits_large_g(G):
    from gm3d_amd.ops import _ptr
    from oracle import hier_ref as HR
    from tests import clouds
    B, radius = 2, 0.32
    gen = torch.Generator().manual_seed(G)
    c = clouds.pc_norm(torch.randn(B, G, 3, generator=gen))
    vis = torch.rand(B, G, generator=gen) < 0.6
    cd, vd = c.cuda(), vis.cuda()
    want = _packed_radius_mask(cd, vd, radius)
    # the reference builder agrees with hier_ref.far_mask + ops.pack_mask where both fit
    from gm3d_amd import ops
    cs, vs = c[:1, :300], vis[:1, :300]
    small = ~(vs[:, :, None] & vs[:, None, :]) | HR.far_mask(cs, radius)
    assert torch.equal(_packed_radius_mask(cs.cuda(), vs.cuda(), radius), ops.pack_mask(small.cuda()))
    W = (G + 31) // 32
    bits = Guarded((B, G, W), torch.int32, I32_SENT)
    flags = vd.to(torch.uint8)
    _ok(_lib().gm3d_radius_mask_bits_m(_ptr(cd), _ptr(flags), 0, radius, B, G, _ptr(bits.t), None), "radius_mask_bits")
    torch.cuda.synchronize()
    assert bool((bits.buf[bits.n:] == I32_SENT).all()), "write past the end"
    assert torch.equal(bits.t, want)


# ------------------------------------------------------------------ gathers, partition, back-projection at their maxima
def test_gather_points_grad_max_m():
    from gm3d_amd.ops import _ptr
    B, C, N, M = 2, 3, 2048, 16384
    gen = torch.Generator().manual_seed(11)
    idx = torch.randint(0, N, (B, M), generator=gen, dtype=torch.int32)
    gout = torch.randint(-8, 9, (B, C, M), generator=gen).float()        # small integers: every sum is exact in any order
    want = torch.zeros(B, C, N, dtype=torch.float64).scatter_add_(2, idx.long().unsqueeze(1).expand(-1, C, -1), gout.double())
    gf = Guarded((B, C, N), torch.float32, NAN)
    gd, idd = gout.cuda(), idx.cuda()
    _ok(_lib().gm3d_gather_points_grad(_ptr(gd), _ptr(idd), B, C, N, M, _ptr(gf.t), None), "gather_points_grad")
    assert torch.equal(gf.check("grad_feat").cpu().double(), want)


def test_gather_inverse_max_s_and_j():
    from gm3d_amd.ops import _ptr
    B, J, S = 2, 16384, 4096
    gen = torch.Generator().manual_seed(12)
    idx = torch.randint(0, S - 7, (B, J), generator=gen)             # the last sources are never referenced: empty lists
    off = Guarded((B, S + 1), torch.int32, I32_SENT)
    lst = Guarded((B, J), torch.int32, I32_SENT)
    idd = idx.cuda()
    _ok(_lib().gm3d_gather_inverse(_ptr(idd), B, J, S, _ptr(off.t), _ptr(lst.t), None), "gather_inverse")
    counts = torch.stack([torch.bincount(idx[b], minlength=S) for b in range(B)])
    want_off = torch.cat([torch.zeros(B, 1, dtype=torch.long), counts.cumsum(1)], 1)
    want_list = torch.sort(idx, dim=1, stable=True).indices          # by source, ascending j within each source
    assert torch.equal(off.check("off").cpu().long(), want_off)
    assert torch.equal(lst.check("list").cpu().long(), want_list)


@pytest.mark.parametrize("Tc", [1024, 300])
def test_partition_visible_1024_thread_block(Tc):
    from gm3d_amd.ops import _ptr
    B, T = 3, 1024
    gen = torch.Generator().manual_seed(Tc)
    masked = torch.rand(B, T, generator=gen) < 0.75
    for b in range(B):
        v = (~masked[b]).nonzero().flatten()
        if len(v) > Tc:
            masked[b, v[Tc:]] = True
    md = masked.cuda().to(torch.uint8)
    perm_c, perm_v = Guarded((B, Tc), torch.int32, I32_SENT), Guarded((B, Tc), torch.int32, I32_SENT)
    inv_v, inv_m = Guarded((B, T), torch.int32, I32_SENT), Guarded((B, T), torch.int32, I32_SENT)
    vis_c = Guarded((B, Tc), torch.uint8, 171)
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ok(_lib().gm3d_partition_visible(_ptr(md), B, T, Tc, _ptr(perm_c.t), _ptr(perm_v.t), _ptr(inv_v.t), _ptr(inv_m.t), _ptr(vis_c.t),
                                      _ptr(overflow), None), "partition_visible")
    got = {k: g.check(k).cpu().long() for k, g in (("perm_c", perm_c), ("perm_v", perm_v), ("inv_v", inv_v), ("inv_m", inv_m),
                                                    ("vis_c", vis_c))}
    assert int(overflow) == 0
    for b in range(B):
        v = (~masked[b]).nonzero().flatten()
        m = masked[b].nonzero().flatten()
        order = torch.cat([v, m])[:Tc]
        assert torch.equal(got["perm_c"][b], order)
        want_v = order.clone()
        want_v[len(v):] = -1
        assert torch.equal(got["perm_v"][b], want_v)
        inv = torch.full((T,), -1, dtype=torch.long)
        inv[v] = torch.arange(len(v))
        assert torch.equal(got["inv_v"][b], inv)
        assert torch.equal(got["inv_m"][b], torch.where(masked[b], torch.arange(T), torch.tensor(-1)))
        assert torch.equal(got["vis_c"][b], (torch.arange(Tc) < len(v)).long())


def test_back_project_max_gf():
    from gm3d_amd import point_m2ae as P
    from gm3d_amd.ops import _ptr
    B, Gc, k, Gf = 2, 512, 8, 8192
    gen = torch.Generator().manual_seed(13)
    member = torch.randint(0, Gf, (B, Gc, k), generator=gen)
    coarse = torch.rand(B, Gc, generator=gen) < 0.5
    want = P.back_project(coarse, [torch.zeros(B, Gf, 1, dtype=torch.long), member])[0]      # CPU: integer scatter-add form
    out = Guarded((B, Gf), torch.uint8, 171)
    cd, md = coarse.cuda().to(torch.uint8), member.cuda()
    _ok(_lib().gm3d_back_project(_ptr(cd), _ptr(md), B, Gc, k, Gf, _ptr(out.t), None), "back_project")
    assert torch.equal(out.check("masked_f").cpu().bool(), want)
    assert 0 < int(want.sum()) < B * Gf


# ------------------------------------------------------------------ GELU backward reductions at their widest rows
@pytest.mark.parametrize("adt,tol", [(torch.float32, 1e-5), (torch.bfloat16, 1.2e-2)])
def test_bias_gelu_bwd_c8192(adt, tol):
    from gm3d_amd import fused
    import torch.nn.functional as F
    R, C = 37, 8192
    torch.manual_seed(C)
    f = (torch.randn(R, C, device="cuda") * 2).to(adt)
    bias = torch.randn(C, device="cuda") * 0.5
    dg = torch.randn(R, C, device="cuda").to(adt)
    g = Guarded((R, C), adt, NAN)
    fused.bias_gelu_fwd(f, bias, adt, g=g.t)
    df = Guarded((R, C), adt, NAN)
    df_t, db = fused.bias_gelu_bwd(dg, f, bias, adt, df=df.t)
    assert df_t.data_ptr() == df.t.data_ptr()
    pre = (f.double() + bias.double()).requires_grad_(True)
    ref = F.gelu(pre)
    assert rel(g.check("g"), ref.detach()) <= tol
    ref.backward(dg.double())
    assert rel(df.check("df"), pre.grad) <= tol
    assert rel(db, pre.grad.sum(0)) <= 2e-5


@pytest.mark.parametrize("C", [256, 512])
def test_lin3_gelu_bwd_at_64_kib_tile(C):
    """gm3d_lin3_gelu_bwd at C = 256 (8 slices) and C = 512 (4 slices): both an fp64 LDS tile of exactly 64 KiB."""
    from gm3d_amd.ops import _ptr
    import torch.nn.functional as F
    lib = _lib()
    R = 5000
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(R, 3, generator=gen)
    w = torch.randn(C, 3, generator=gen) * 0.7
    b = torch.randn(C, generator=gen) * 0.2
    dout = torch.randn(R, C, generator=gen)
    xd, wd, bd, dd = x.cuda(), w.cuda(), b.cuda(), dout.cuda()
    nrows = lib.gm3d_embed_partial_rows(3, R, C)
    part = Guarded((nrows, 4 * C), torch.float64, NAN)
    _ok(lib.gm3d_lin3_gelu_bwd(_ptr(dd), _ptr(xd), _ptr(wd), _ptr(bd), R, C, _ptr(part.t), 0, None), "lin3_gelu_bwd")
    part.check("partial")
    dW = Guarded((C, 3), torch.float32, NAN)
    db = Guarded((C,), torch.float32, NAN)
    _ok(lib.gm3d_lin3_finish(_ptr(part.t), nrows, C, _ptr(dW.t), _ptr(db.t), None), "lin3_finish")
    x64, w64, b64 = x.double(), w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.gelu(x64 @ w64.t() + b64).backward(dout.double())
    assert rel(dW.check("dW"), w64.grad) <= 1e-5 and rel(db.check("db"), b64.grad) <= 1e-5


# ------------------------------------------------------------------ the embed's layer-1 backward statistics at C1 around 200 .. 256
def _encoder_fp64(enc, nb, arg1, arg2):
    """Encoder.forward (train mode: BatchNorm on batch statistics) restated in fp64 on an fp64 copy of its parameters, its two
    max-pools taking the rows arg1 (groups, 256) / arg2 (groups, C) name.  -> (tokens, [(pre-pool, arg), ...])."""
    import torch.nn.functional as F
    c0, bn0, _, c1 = enc.first_conv
    c2, bn1, _, c3 = enc.second_conv
    bs, g, n, _ = nb.shape
    x = nb.reshape(-1, 3)
    bn = lambda t, m: F.batch_norm(t, None, None, m.weight, m.bias, True, 0.0, m.eps)
    h = F.relu(bn(F.linear(x, c0.weight.squeeze(-1), c0.bias), bn0))
    f = F.linear(h, c1.weight.squeeze(-1), c1.bias).view(bs * g, n, -1)
    fg = f.gather(1, arg1.long().unsqueeze(1)).squeeze(1)
    w2 = c2.weight.squeeze(-1)
    y = torch.cat([fg.unsqueeze(1).expand(-1, n, -1), f], -1).reshape(bs * g * n, -1)
    y = F.relu(bn(F.linear(y, w2, c2.bias), bn1))
    z = F.linear(y, c3.weight.squeeze(-1), c3.bias).view(bs * g, n, -1)
    return z.gather(1, arg2.long().unsqueeze(1)).squeeze(1).view(bs, g, -1), [(f, arg1), (z, arg2)]


@pytest.mark.parametrize("C1", [128, 200, 208, 256])
def test_embed_layer1_width(C1):
    """EmbedFn with a first conv of C1 channels: its backward runs gm3d_pn_layer1_bwd_stats with 8 row slices up to C1 = 200 and
    4 above (the fp64 LDS tile stays within 64 KiB).  fp32 tokens and every parameter gradient against an fp64 restatement of the
    module at the bars of test_gpu_embed.py (C1 = 128, the model's width, is the control).
    The two max-pools decide discretely: with 32 rows per group the top two of a (group, channel) are often within 1e-7 of the
    scale, inside fp32 rounding, and the fused path (BatchNorm folded into the first conv) may pick either.  One such pick moves
    every gradient by 1e-3 .. 1e-2 (C1 = 256 with this seed).  So the reference pools take the rows the kernels chose, after
    checking that each chosen row holds the fp64 maximum to within fp32 rounding."""
    from gm3d_amd import models_mae_learn_loss as M
    from tests.test_gpu_embed import _err
    torch.manual_seed(C1)
    base = M.Encoder(384)
    base.first_conv = torch.nn.Sequential(torch.nn.Conv1d(3, C1, 1), torch.nn.BatchNorm1d(C1), torch.nn.ReLU(inplace=True),
                                          torch.nn.Conv1d(C1, 256, 1))
    base = base.cuda()
    with torch.no_grad():
        for m in base.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
    B, G = 2, 64
    nb = torch.randn(B, G, 32, 3, device="cuda") * 0.2
    w = torch.randn(B, G, 384, device="cuda")
    enc = copy.deepcopy(base).train()
    assert M.FUSED_EMBED and enc.fused(nb)
    tok = enc(nb)
    node = tok.grad_fn
    while "EmbedFn" not in type(node).__name__:
        node = node.next_functions[0][0]
    saved = node.saved_tensors               # (x, a1, f, fg, arg1, y0, t, a2, arg2, ...): EmbedFn._forward's save_for_backward
    arg1, arg2 = saved[4], saved[8]
    assert arg1.shape == (B * G, 256) and arg2.shape == (B * G, 384) and arg1.dtype == arg2.dtype == torch.uint8
    (tok.float() * w).sum().backward()
    g = {k: p.grad.detach().double() for k, p in enc.named_parameters()}
    e64 = copy.deepcopy(base).double()
    ref_tok, pools = _encoder_fp64(e64, nb.double(), arg1, arg2)
    for pre, arg in pools:
        pre = pre.detach()
        chosen = pre.gather(1, arg.long().unsqueeze(1)).squeeze(1)
        assert float((pre.amax(1) - chosen).max()) <= 1e-6 * float(pre.abs().max())        # a maximum, up to fp32 rounding
    (ref_tok * w.double()).sum().backward()
    ref_g = {k: p.grad.detach() for k, p in e64.named_parameters()}
    assert _err(tok.detach().double(), ref_tok.detach()) <= 1e-5 * float(ref_tok.detach().abs().max())
    gnorm = sum(float(v.pow(2).sum()) for v in ref_g.values()) ** 0.5
    for k in ref_g:
        assert _err(g[k], ref_g[k]) <= 3e-5 * float(ref_g[k].abs().max()) + 1e-6 * gnorm, (k, _err(g[k], ref_g[k]))


# ------------------------------------------------------------------ classification tail: V up to 16 (LDS above 64 KiB), cls_dim 1 / 256
@pytest.mark.parametrize("V", [1, 15, 16])
@pytest.mark.parametrize("cls_dim", [1, 256])
def test_cls_tail_vote_edges(V, cls_dim):
    from gm3d_amd import ops
    from tests.test_gpu_vote import _head
    B, T = 3, 2
    head = _head(cls_dim, seed=V * 7 + cls_dim)
    g = torch.Generator(device="cuda").manual_seed(V * 1000 + cls_dim)
    x = torch.randn(V * B, T, 384, device="cuda", generator=g)
    h64 = copy.deepcopy(head).double()
    with torch.no_grad():
        want = h64(torch.cat([x[:, 0], x[:, 1:].max(1)[0]], dim=-1).double()).view(V, B, cls_dim)
    labels = torch.zeros(B, dtype=torch.long, device="cuda")
    correct = torch.zeros(1, dtype=torch.long, device="cuda")
    for dt in (torch.float32, torch.bfloat16):
        xx = x.to(dt)
        if dt == torch.bfloat16:
            with torch.no_grad():
                want = h64(torch.cat([xx[:, 0], xx[:, 1:].max(1)[0]], dim=-1).double()).view(V, B, cls_dim)
        votes = Guarded((V, B, cls_dim), torch.float32, NAN)
        correct.zero_()
        mean, pred = ops.cls_tail_vote(xx, head, labels, V, correct, votes=votes.t)
        assert rel(votes.check("votes"), want) <= 1e-5, dt
        assert rel(mean, want.sum(0) / V) <= 1e-5
        assert torch.equal(pred, mean.argmax(-1))
        assert int(correct) == int((pred == labels).sum())


# ------------------------------------------------------------------ weight gradients on 128 x 384 tiles: one whole tile, one stage per split
@pytest.mark.parametrize("nb,R,N,K,splits", [(1, 32, 128, 384, 1), (2, 128, 128, 384, 4), (1, 64, 256, 768, 2), (3, 4096, 128, 384, 1)])
def test_gemm_nt_big_tiles_smallest_shapes(nb, R, N, K, splits):
    """gm3d_gemm_nt_bf16_big at the smallest (N, K) its guard accepts -- one 128 x 384 tile -- and with a single 32-row stage per row
    split, through the raw entry point into a guarded slab buffer: the slab sum against an fp32 torch.bmm of the same bf16 operands at
    the bar of test_gemm_nt_weight_gradient (fp32 accumulation error only)."""
    from gm3d_amd.ops import _ptr
    g = torch.Generator(device="cuda").manual_seed(R + N + K + splits)
    dy = torch.randn(nb, R, N, device="cuda", generator=g).bfloat16()
    x = torch.randn(nb, R, K, device="cuda", generator=g).bfloat16()
    part = Guarded((nb, splits, N, K), torch.float32, NAN)
    _ok(_lib().gm3d_gemm_nt_bf16_big(_ptr(dy), _ptr(x), _ptr(part.t), nb, R, N, K, N, K, K, R * N, R * K, splits * N * K, splits, N * K,
                                     None), "gm3d_gemm_nt_bf16_big")
    got = part.check("slabs").sum(1)
    want = torch.bmm(dy.float().transpose(1, 2), x.float())
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()) * max(1.0, (R / 4096) ** 0.5)

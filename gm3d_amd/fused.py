"""Fused transformer stack: the blocks of TransformerEncoder / TransformerDecoder plus their final LayerNorm
as ONE autograd node with a hand-written forward and backward.

Restates, operation for operation, timm-0.4.5 Block (in-tree twin Point-MAE_SA3D/models/Point_MAE.py:82-146)
as driven by P/models_mae_learn_loss.py:914-917 and :984-990:

    for block in blocks:  x = block(x + pos)        # x += dp(attn(LN1(x)));  x += dp(mlp(LN2(x)))
    return LayerNorm(x)

Per block the forward is 4 GEMMs (the MFMA kernels of csrc/gemm*.hip through gemm.mm, on cached bf16 weights), the MFMA attention kernel and
3 row-wise HIP passes (gm3d_amd/csrc/rowops.hip): [residual + bias + DropPath + pos + LayerNorm] x2 and
[bias + GELU]; the backward is 8 GEMMs, the attention backward and 3 row-wise passes that also produce every
bias / gamma / beta gradient as fused column sums.  The residual stream is fp32, GEMM operands are bf16
(throughput mode) or fp32 (parity mode: same code path, checked to 1e-5 against the reference fixtures).
"""
import weakref

import torch

from ._capi import lib
from . import attention, gemm, wgrads
from . import streams as _streams
from .gemm import bias_gelu_bwd, bias_gelu_fwd  # noqa: F401  (their home is beside the products they follow)
from .ops import _launch, _ptr, _stream, _DT
from .wgrads import async_wgrad, defer_wgrad  # noqa: F401  (INTEGRATION.md and the engines name them here)

LNC = 384


# ----------------------------------------------------------------------------- bf16 weight cache
class _WeightCache:
    """bf16 copies of the 2-D fp32 master weights for the GEMMs.

    * `pin(model)` / `refresh()`: persistent bf16 buffers for every >=2-D parameter of a model, re-cast by ONE
      multi-tensor launch (the engine calls refresh() once per step for student and teacher; autocast re-casts
      ~400 times per step).  Under hipGraph capture this is the only mode that is correct: the refresh launch is
      part of the captured step, and get() involves no host-side staleness decision.
    * un-pinned weights: cached per (storage, version counter); re-cast when the master changed; never cached
      while a stream capture is running."""

    def __init__(self):
        self._c = {}
        self._pinned = {}      # data_ptr -> bf16 buffer
        self._groups = []      # (fp32 list, bf16 list)

    def pin(self, model, dtype=torch.bfloat16, static=False):
        """static=True: frozen weights -- cast once, never re-cast by refresh()."""
        src = [p for p in model.parameters() if p.dim() >= 2 and p.dtype == torch.float32 and p.is_cuda
               and not self._is_pinned(p)]
        if not src:
            return
        dst = [torch.empty_like(p, dtype=dtype) for p in src]
        for p, d in zip(src, dst):
            self._pinned[p.data_ptr()] = (d, weakref.ref(p))
        if static:
            with torch.no_grad():
                torch._foreach_copy_(dst, [p.detach() for p in src])
            return
        self._groups.append(([p.detach() for p in src], dst))
        with torch.no_grad():
            torch._foreach_copy_(dst, self._groups[-1][0])

    def pin_view(self, p, shadow):
        """Register an externally maintained bf16 copy of `p` (FlatAdamWEma rewrites it inside its update kernel)."""
        self._pinned[p.data_ptr()] = (shadow, weakref.ref(p))
        gemm.forget_transposes()        # shadows of another optimizer: whatever mm_nn remembered is stale

    def _is_pinned(self, p):
        hit = self._pinned.get(p.data_ptr())
        return hit is not None and hit[1]() is p

    def refresh(self):
        with torch.no_grad():
            for src, dst in self._groups:
                torch._foreach_copy_(dst, src)

    def get(self, w, dtype):
        if w.dtype == dtype:
            return w
        hit = self._pinned.get(w.data_ptr())
        if hit is not None and hit[1]() is w and hit[0].dtype == dtype:
            return hit[0]
        base = w._base
        if base is not None and base.dtype == w.dtype:
            # a view of a pinned parameter (the [global | local] column halves of a mini-PointNet conv): the same view of its shadow
            hit = self._pinned.get(base.data_ptr())
            if hit is not None and hit[1]() is base and hit[0].dtype == dtype and hit[0].numel() == base.numel():
                return torch.as_strided(hit[0], w.size(), w.stride(), hit[0].storage_offset() + w.storage_offset() - base.storage_offset())
        if torch.cuda.is_current_stream_capturing():
            return w.detach().to(dtype)
        key = (w.data_ptr(), dtype, tuple(w.shape))
        hit = self._c.get(key)
        if hit is not None and hit[0] == w._version and hit[2]() is w:   # same live tensor, unchanged since the cast
            if w.is_cuda:
                # the cast may have been launched on ANOTHER stream a moment ago (the parallel inference chains of run_stack meet the
                # same weights one after the other): whoever reuses it waits for the casting launch and keeps the allocator informed
                cur = torch.cuda.current_stream(w.device)
                if hit[3] != cur.cuda_stream:
                    cur.wait_event(hit[4])
                    hit[1].record_stream(cur)
            return hit[1]
        with torch.no_grad():
            c = w.detach().to(dtype)
        if len(self._c) > 4096:
            self._c.clear()
        stream_id, done = None, None
        if w.is_cuda:
            cur = torch.cuda.current_stream(w.device)
            stream_id, done = cur.cuda_stream, torch.cuda.Event()
            done.record(cur)
        self._c[key] = (w._version, c, weakref.ref(w), stream_id, done)
        return c


weight_cache = _WeightCache()


# ----------------------------------------------------------------------------- row-op wrappers
def residual_ln_fwd(res, y, bias, rowscale, rows_per_sample, add, gamma, beta, eps, adt, R, want_res=True, h=None):
    dev = gamma.device
    out_res = torch.empty(R, LNC, dtype=torch.float32, device=dev) if want_res else None
    if h is None:
        h = torch.empty(R, LNC, dtype=adt, device=dev)
    mean = torch.empty(R, dtype=torch.float32, device=dev)
    rstd = torch.empty(R, dtype=torch.float32, device=dev)
    _launch("gm3d_residual_ln_fwd", {"R": R, "dtype": str(adt)}, lib.gm3d_residual_ln_fwd, _ptr(res), _ptr(y), _ptr(bias),
            _ptr(rowscale), int(rows_per_sample), _ptr(add), _ptr(gamma), _ptr(beta), float(eps), _ptr(out_res), _ptr(h),
            _ptr(mean), _ptr(rstd), R, LNC, _DT[adt], _stream())
    return out_res, h, mean, rstd


def residual_ln_bwd(dh, gin, x, mean, rstd, gamma, rowscale, rows_per_sample, acc, want_dy, adt, R, dy=None, partial=None,
                    acc_out=None):
    """-> dx (R,C) f32, dy (R,C) adt | None, sums (3,C) f32 = [dgamma, dbeta, colsum(dy)].
    With `partial` given (a (rows, 3C) slice of a batched buffer) the second stage is left to the caller.
    acc_out (R,C) adt: receives the updated `acc` in the activation type too."""
    dev = gamma.device
    dx = torch.empty(R, LNC, dtype=torch.float32, device=dev)
    if dy is None and want_dy:
        dy = torch.empty(R, LNC, dtype=adt, device=dev)
    nrows = lib.gm3d_ln_partial_rows(R)
    defer = partial is not None
    if partial is None:
        partial = torch.empty(nrows, 3 * LNC, dtype=torch.float32, device=dev)
    _launch("gm3d_residual_ln_bwd", {"R": R, "dtype": str(adt)}, lib.gm3d_residual_ln_bwd, _ptr(dh), _ptr(gin), _ptr(x),
            _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(rowscale), int(rows_per_sample), _ptr(dx), _ptr(dy), _ptr(acc),
            _ptr(acc_out), _ptr(partial), R, LNC, _DT[adt], _stream())
    if defer:
        return dx, dy, None
    sums = torch.empty(3, LNC, dtype=torch.float32, device=dev)
    _launch("gm3d_colsum_finish", {"rows": nrows, "cols": 3 * LNC}, lib.gm3d_colsum_finish, _ptr(partial), nrows, 3 * LNC,
            3 * LNC, _ptr(sums), 0, _stream())
    return dx, dy, sums


def finish_batched(partial, out):
    """partial (J, rows, cols) f32 -> out (J, cols): every job's second stage in one launch."""
    J, rows, cols = partial.shape
    _launch("gm3d_colsum_finish_batched", {"rows": J * rows, "cols": cols}, lib.gm3d_colsum_finish_batched, _ptr(partial), J,
            rows * cols, rows, cols, cols, _ptr(out), cols, _stream())
    return out


DIRECT_INPUT_GRADS = True   # the stack backward writes dx / dpos in the activation type itself (no converting copies)
FUSE_QKV_ATTENTION = True   # qkv GEMM + attention forward as one launch (bf16, 32 < T <= 64)
PER_BLOCK = 11  # ln1.w ln1.b qkv.w proj.w proj.b ln2.w ln2.b fc1.w fc1.b fc2.w fc2.b


def block_params(block):
    return [block.norm1.weight, block.norm1.bias, block.attn.qkv.weight, block.attn.proj.weight, block.attn.proj.bias,
            block.norm2.weight, block.norm2.bias, block.mlp.fc1.weight, block.mlp.fc1.bias, block.mlp.fc2.weight,
            block.mlp.fc2.bias]


class TransformerStackFn(torch.autograd.Function):
    """args: x (B,T,C), pos (B,T,C), meta, final_w, final_b, then PER_BLOCK tensors per block.
    meta: dict(num_heads, scale, eps, final_eps, adt, dp=[(scale_attn|None, scale_mlp|None) per block])."""

    @staticmethod
    def forward(ctx, x, pos, meta, final_w, final_b, *params):
        with torch.autocast("cuda", enabled=False):
            return TransformerStackFn._forward(ctx, x, pos, meta, final_w, final_b, *params)

    @staticmethod
    def _forward(ctx, x, pos, meta, final_w, final_b, *params):
        g = TransformerStackFn._forward_gen(ctx, x, pos, meta, final_w, final_b, *params)
        while True:
            try:
                next(g)
            except StopIteration as done:
                return done.value

    @staticmethod
    def _forward_gen(ctx, x, pos, meta, final_w, final_b, *params):
        """The forward as a generator that yields after every kernel launch: run_stack drives several half-batch chains in
        lock-step, one launch of each in turn on its own stream, so that a captured graph holds them as interleaved branches."""
        B, T, C = x.shape
        assert C == LNC and len(params) % PER_BLOCK == 0
        nblk = len(params) // PER_BLOCK
        adt, H, scale, eps = meta["adt"], meta["num_heads"], meta["scale"], meta["eps"]
        R = B * T
        posa = pos.reshape(R, C).to(adt).contiguous()
        need = meta["grad"] and any(ctx.needs_input_grad)   # grad mode is off inside forward: captured by run_stack
        y = bias = rs = None
        if x.dtype == adt and adt != torch.float32:
            # tokens already in the activation dtype: the first LayerNorm pass reads them as its branch operand (u = x + pos) --
            # no fp32 copy of the input
            res, y = None, x.reshape(R, C).contiguous()
        else:
            res = x.reshape(R, C).float().contiguous()
        saved = []
        dev = x.device
        if need:  # operands of the weight-gradient GEMMs, stacked over blocks for the batched wgrad
            H1 = torch.empty(nblk, R, C, dtype=adt, device=dev)
            A = torch.empty(nblk, R, C, dtype=adt, device=dev)
            H2 = torch.empty(nblk, R, C, dtype=adt, device=dev)
            GG = torch.empty(nblk, R, 4 * C, dtype=adt, device=dev)
        # LayerNorm folded into the GEMMs around it (bf16 path): proj / fc2 write the fp32 residual stream + per-tile row
        # statistics in their epilogue (gm3d_gemm_tn_bf16_res), qkv / fc1 normalise while they stage their A operand
        # (gm3d_gemm_tn_bf16_lna).  Stand-alone LayerNorm passes remain only in front of the first block and behind the last.
        fuse_ln = (gemm.fuse_ln() and adt == torch.bfloat16 and x.is_cuda
                   and all(gemm.supported(posa, weight_cache.get(params[i * PER_BLOCK + k], adt)) or k == 9
                           for i in range(nblk) for k in (2, 3, 7)))
        st1 = None
        for i in range(nblk):
            ln1w, ln1b, wqkv, wproj, bproj, ln2w, ln2b, w1, b1, w2, b2 = params[i * PER_BLOCK:(i + 1) * PER_BLOCK]
            dp1, dp2 = meta["dp"][i]
            if fuse_ln:
                if i == 0:
                    u, h1, m1, r1 = residual_ln_fwd(res, y, bias, rs, T, posa, ln1w, ln1b, eps, adt, R, h=H1[i] if need else None)
                    yield
                    qkv = gemm.mm(h1, weight_cache.get(wqkv, adt))
                else:       # u, st1: the previous block's fc2 epilogue
                    qkv, m1, r1 = gemm.linear_lna(u16, st1, ln1w, ln1b, eps, weight_cache.get(wqkv, adt), None,
                                                  h_out=H1[i] if need else None, want_stats=need)
                yield
                a, lse = attention.fwd(qkv, None, B, T, H, 64, scale, out=A[i] if need else None, head=True, pad=True)
                yield
                x1, x16, st2 = gemm.linear_res(a, weight_cache.get(wproj, adt), bproj, u, dp1, T, None)
                yield
                W1 = weight_cache.get(w1, adt)
                f, g, m2, r2 = gemm.linear_lna(x16, st2, ln2w, ln2b, eps, W1, b1, gelu=True,
                                               f_out=torch.empty(R, W1.shape[0], dtype=adt, device=dev) if need else None,
                                               g_out=GG[i] if need else None, h_out=H2[i] if need else None, want_stats=need)
                yield
                if need:
                    saved += [u, m1, r1, qkv, lse, x1, m2, r2, f]
                if i + 1 < nblk:
                    u, u16, st1 = gemm.linear_res(g, weight_cache.get(w2, adt), b2, x1, dp2, T, posa)
                else:
                    o = gemm.mm(g, weight_cache.get(w2, adt))
                    res, y, bias, rs = x1, o, b2, dp2
                yield
                continue
            u, h1, m1, r1 = residual_ln_fwd(res, y, bias, rs, T, posa, ln1w, ln1b, eps, adt, R, h=H1[i] if need else None)
            yield
            Wq = weight_cache.get(wqkv, adt)
            if attention.route_qkv(h1, Wq, T, H, FUSE_QKV_ATTENTION):
                # q|k|v never leave the CU in the no-grad (teacher) pass; with a backward to come they are written on the side
                a, lse, qkv = attention.qkv_fwd(h1, Wq, B, T, H, scale, out=A[i] if need else None, want_qkv=need, want_lse=need)
            else:
                qkv = gemm.mm(h1, Wq)
                yield
                a, lse = attention.fwd(qkv, None, B, T, H, 64, scale, out=A[i] if need else None, head=True, pad=True)
            yield
            p = gemm.mm(a, weight_cache.get(wproj, adt))
            yield
            x1, h2, m2, r2 = residual_ln_fwd(u, p, bproj, dp1, T, None, ln2w, ln2b, eps, adt, R, h=H2[i] if need else None)
            yield
            W1 = weight_cache.get(w1, adt)
            if gemm.route_gelu(h2, W1)[0] == "split":      # two launches: run here, for the yield between them
                f = gemm.mm(h2, W1)
                yield
                g = bias_gelu_fwd(f, b1, adt, g=GG[i] if need else None)
            else:
                # fc1 + bias + GELU in the GEMM epilogue; the pre-activation is only written when a backward follows
                f, g = gemm.mm_gelu(h2, W1, b1, need, g_out=GG[i] if need else None)
            yield
            o = gemm.mm(g, weight_cache.get(w2, adt))
            yield
            if need:
                saved += [u, m1, r1, qkv, lse, x1, m2, r2, f]
            res, y, bias, rs = x1, o, b2, dp2
        xf, hout, mf, rf = residual_ln_fwd(res, y, bias, rs, T, None, final_w, final_b, meta["final_eps"], adt, R,
                                           want_res=need, h=meta.get("hout"))
        if need:
            ctx.save_for_backward(final_w, xf, mf, rf, H1, A, H2, GG, *params, *saved)
        ctx.meta, ctx.shape, ctx.nblk = meta, (B, T, C), nblk
        ctx.in_dtypes = (x.dtype, pos.dtype)
        return hout.view(B, T, C)

    @staticmethod
    def backward(ctx, dout):
        with torch.autocast("cuda", enabled=False):
            return TransformerStackFn._backward(ctx, dout)

    @staticmethod
    def _backward(ctx, dout):
        meta, (B, T, C), nblk = ctx.meta, ctx.shape, ctx.nblk
        adt, H, scale = meta["adt"], meta["num_heads"], meta["scale"]
        R = B * T
        tens = ctx.saved_tensors
        final_w, xf, mf, rf, H1, A, H2, GG = tens[:8]
        params = tens[8:8 + nblk * PER_BLOCK]
        saved = tens[8 + nblk * PER_BLOCK:]
        grads = [None] * (nblk * PER_BLOCK)
        dev = dout.device
        dh = dout.reshape(R, C).to(adt).contiguous()
        # output-side operands of the weight-gradient GEMMs, stacked over blocks
        DO = torch.empty(nblk, R, C, dtype=adt, device=dev)
        DF = torch.empty(nblk, R, 4 * C, dtype=adt, device=dev)
        DP = torch.empty(nblk, R, C, dtype=adt, device=dev)
        DQ = torch.empty(nblk, R, 3 * C, dtype=adt, device=dev)
        # column-sum partials of every LayerNorm site (job 2i: LN1 of block i, 2i+1: LN2, 2*nblk: final) and of every
        # GELU site, finished by ONE launch each after the loop
        PLN = torch.empty(2 * nblk + 1, lib.gm3d_ln_partial_rows(R), 3 * C, dtype=torch.float32, device=dev)
        SLN = torch.empty(2 * nblk + 1, 3, C, dtype=torch.float32, device=dev)
        # fc2 input gradient + GELU backward + fc1 bias-gradient partials as ONE launch of the hand-written GEMM (bf16 path):
        # it wants fc2.weight^T (and proj.weight^T for the attention branch), produced for the whole stack by one strided
        # transposing copy each from the optimizer's flat bf16 shadow
        w2s = [weight_cache.get(params[i * PER_BLOCK + 9], adt) for i in range(nblk)]
        gelu_bwd = gemm.route_gelu_bwd(dh, w2s[0])
        fuse_mlp_bwd = gelu_bwd[0] != "split"
        if fuse_mlp_bwd:
            # fc2^T (nblk, 4C, C), proj^T (nblk, C, C) and -- fc1 / qkv input gradients as TN products on the LDS-DMA ring kernel (N = 384
            # columns, K = 1536 / 1152: its regime) -- fc1^T (nblk, C, 4C), qkv^T (nblk, C, 3C): ONE transposing launch for the four
            W2T, WPT, W1T, WQT = gemm.stacked_transposes(
                [w2s] + [[weight_cache.get(params[i * PER_BLOCK + k], adt) for i in range(nblk)] for k in (3, 7, 2)])
        PGL = torch.empty(nblk, gelu_bwd[2], 4 * C, dtype=torch.float32, device=dev)
        SGL = torch.empty(nblk, 4 * C, dtype=torch.float32, device=dev)
        dp2_last = meta["dp"][nblk - 1][1]
        G, d_o, _ = residual_ln_bwd(dh, None, xf, mf, rf, final_w, dp2_last, T, None, True, adt, R, dy=DO[nblk - 1],
                                    partial=PLN[2 * nblk])
        g_final_w, g_final_b, db2 = SLN[2 * nblk, 0], SLN[2 * nblk, 1], SLN[2 * nblk, 2]
        # gradient of the positional embedding = sum over blocks of the gradient at every u = x + pos site.  The first site's gradient
        # (G of the last block) starts the sum: that buffer's only other reader, the next block's LayerNorm-2 backward, has run
        # by the time the next site accumulates into it -- no zero fill, no read-modify-write for the first site.
        dpos = torch.zeros(R, C, dtype=torch.float32, device=dev) if nblk == 1 else None
        for i in range(nblk - 1, -1, -1):
            ln1w, ln1b, wqkv, wproj, bproj, ln2w, ln2b, w1, b1, w2, b2 = params[i * PER_BLOCK:(i + 1) * PER_BLOCK]
            u, m1, r1, qkv, lse, x1, m2, r2, f = saved[i * 9:(i + 1) * 9]
            dp1 = meta["dp"][i][0]
            dp2_prev = meta["dp"][i - 1][1] if i > 0 else None
            gi = grads[i * PER_BLOCK:(i + 1) * PER_BLOCK]
            # mlp branch: x2 = x1 + dp2 * (g @ W2^T + b2)
            gi[10] = db2
            if fuse_mlp_bwd:
                df = gemm.mm_gelu_bwd(d_o, W2T[i], f, b1, DF[i], PGL[i], gelu_bwd)
            else:
                dg = gemm.mm_nn(d_o, weight_cache.get(w2, adt))
                df, _ = bias_gelu_bwd(dg, f, b1, adt, df=DF[i], partial=PGL[i])
            gi[8] = SGL[i]
            dh2 = gemm.mm(df, W1T[i]) if fuse_mlp_bwd else gemm.mm_nn(df, weight_cache.get(w1, adt))
            dx1, d_p, _ = residual_ln_bwd(dh2, G, x1, m2, r2, ln2w, dp1, T, None, True, adt, R, dy=DP[i],
                                          partial=PLN[2 * i + 1])
            gi[5], gi[6], gi[4] = SLN[2 * i + 1, 0], SLN[2 * i + 1, 1], SLN[2 * i + 1, 2]
            # attention branch: x1 = u + dp1 * (a @ Wproj^T + bproj)
            da = gemm.mm(d_p, WPT[i]) if fuse_mlp_bwd else gemm.mm_nn(d_p, weight_cache.get(wproj, adt))
            dqkv = attention.bwd(qkv, None, A[i], da, lse, B, T, H, 64, scale, dqkv=DQ[i], head=True, pad=True)
            dh1 = gemm.mm(dqkv, WQT[i]) if fuse_mlp_bwd else gemm.mm_nn(dqkv, weight_cache.get(wqkv, adt))
            last = DIRECT_INPUT_GRADS and i == 0 and nblk > 1 and adt != torch.float32 and ctx.in_dtypes == (adt, adt)
            if last:
                # the stack's input gradients in the inputs' own (activation) type, written by this last pass instead of two
                # converting copies behind it: dy = 1 * dx (no DropPath factor in front of block 0), acc_out = the finished dpos
                dx_a = torch.empty(R, C, dtype=adt, device=dev)
                dpos_a = torch.empty(R, C, dtype=adt, device=dev)
                G, _, _ = residual_ln_bwd(dh1, dx1, u, m1, r1, ln1w, None, T, dpos, True, adt, R, dy=dx_a, partial=PLN[0],
                                          acc_out=dpos_a)
            else:
                G, d_o, _ = residual_ln_bwd(dh1, dx1, u, m1, r1, ln1w, dp2_prev, T, dpos, i > 0, adt, R,
                                            dy=DO[i - 1] if i > 0 else None, partial=PLN[2 * i])
            if dpos is None:
                dpos = G
            gi[0], gi[1] = SLN[2 * i, 0], SLN[2 * i, 1]
            db2 = SLN[2 * i, 2]
            grads[i * PER_BLOCK:(i + 1) * PER_BLOCK] = gi
        finish_batched(PLN, SLN.view(2 * nblk + 1, 3 * C))
        finish_batched(PGL, SGL)
        # all weight gradients of the stack: 4 batched GEMMs, forked to the side stream or deferred inside an async_wgrad region
        grads[9::PER_BLOCK], grads[7::PER_BLOCK], grads[3::PER_BLOCK], grads[2::PER_BLOCK] = wgrads.stack(
            [(DO, GG, params[9::PER_BLOCK]), (DF, H2, params[7::PER_BLOCK]), (DP, A, params[3::PER_BLOCK]), (DQ, H1, params[2::PER_BLOCK])],
            takes_part=True)
        if last:
            return (dx_a.view(B, T, C), dpos_a.view(B, T, C), None, g_final_w, g_final_b) + tuple(grads)
        dx = G.view(B, T, C).to(ctx.in_dtypes[0])
        return (dx, dpos.view(B, T, C).to(ctx.in_dtypes[1]), None, g_final_w, g_final_b) + tuple(grads)


def run_stack(blocks, final_norm, x, pos, training):
    """blocks: iterable of Block modules; final_norm: nn.LayerNorm.  x, pos (B,T,384)."""
    from . import models_mae_learn_loss as M  # drop_path_scale lives there (the tests replay recorded draws through it)
    blocks = list(blocks)
    adt = torch.bfloat16 if (torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.bfloat16) \
        or x.dtype == torch.bfloat16 else torch.float32
    B = x.shape[0]
    probs = []
    for b in blocks:
        p = getattr(b.drop_path, "drop_prob", 0.0)
        probs += [p, p]
    scales = M.drop_path_scales(B, probs, training, x.device)
    dp = [(scales[2 * i], scales[2 * i + 1]) for i in range(len(blocks))]
    meta = {"num_heads": blocks[0].attn.num_heads, "scale": blocks[0].attn.scale, "eps": blocks[0].norm1.eps,
            "final_eps": final_norm.eps, "adt": adt, "dp": dp, "grad": torch.is_grad_enabled()}
    params = []
    for b in blocks:
        params += block_params(b)
    ns = NOGRAD_SPLIT
    if (ns > 1 and x.is_cuda and not training and B % ns == 0 and B // ns >= 16
            and not (torch.is_grad_enabled() and (x.requires_grad or params[0].requires_grad))):
        # Inference-only stack (the EMA teacher): nothing couples the clouds of a batch, and even an 8192-row chain of these kernels
        # fills the chip about half -- the batch is cut into `ns` parts that run as parallel chains on their own streams (parallel
        # branches of a captured graph), each kernel on 1/ns of the rows.
        main = torch.cuda.current_stream()
        h = B // ns
        x, pos = x.contiguous(), pos.contiguous()
        outs = [None] * ns
        streams = [main] + [_split_stream(x.device, j) for j in range(1, ns)]
        for side in streams[1:]:
            _streams.fork(side, main, who="fused.run_stack: parallel inference chain (NOGRAD_SPLIT)")
            x.record_stream(side)
            pos.record_stream(side)
        if LOCKSTEP:
            # one launch of every chain in turn: the capture (and the graph executor's enqueue order) interleaves the branches;
            # every chain's final LayerNorm writes its rows of ONE output buffer (no concatenation afterwards)
            T_, C_ = x.shape[1], x.shape[2]
            out = torch.empty(B, T_, C_, dtype=adt, device=x.device)
            for side in streams[1:]:
                out.record_stream(side)
            with torch.autocast("cuda", enabled=False), torch.no_grad():
                gens = [TransformerStackFn._forward_gen(_NoCtx(), x[j * h:(j + 1) * h], pos[j * h:(j + 1) * h],
                                                        dict(meta, hout=out[j * h:(j + 1) * h].view(h * T_, C_)), final_norm.weight,
                                                        final_norm.bias, *params) for j in range(ns)]
                live = ns
                while live:
                    for j in range(ns):
                        if gens[j] is None:
                            continue
                        with torch.cuda.stream(streams[j]):
                            try:
                                next(gens[j])
                            except StopIteration as done:
                                outs[j], gens[j] = done.value, None
                                live -= 1
        else:
            for j in range(1, ns):
                with torch.cuda.stream(streams[j]):
                    outs[j] = TransformerStackFn.apply(x[j * h:(j + 1) * h], pos[j * h:(j + 1) * h], meta, final_norm.weight,
                                                       final_norm.bias, *params)
            outs[0] = TransformerStackFn.apply(x[:h], pos[:h], meta, final_norm.weight, final_norm.bias, *params)
        for j in range(1, ns):
            _streams.join(streams[j], main)
            outs[j].record_stream(main)
        return out if LOCKSTEP else torch.cat(outs, dim=0)
    return TransformerStackFn.apply(x, pos, meta, final_norm.weight, final_norm.bias, *params)


class _NoCtx:
    """stand-in for the autograd context in the inference-only lock-step driver (nothing is saved)."""
    needs_input_grad = ()

    def save_for_backward(self, *a):
        pass


LOCKSTEP = True          # interleave the launches of the parallel inference chains (measured: same speed as chain after chain)
NOGRAD_SPLIT = 2         # parallel chains of an inference-only stack (1 = off; measured 2 > 1 > 3 > 4; tests flip it)
_split_streams = {}


def _split_stream(device, j=1):
    key = (device.type, device.index, j)
    if key not in _split_streams:
        _split_streams[key] = torch.cuda.Stream(device=device)
    return _split_streams[key]

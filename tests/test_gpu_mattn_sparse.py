"""-m gpu: both masked-attention kernel pairs (gm3d_amd/csrc/attention_masked.hip through ops.attention_masked, lse through
gm3d_attention_masked_fwd) against the fp64 reference of tests/mattn_ref.py, under masks and values chosen so that each guard of
the flash-style bf16 pair is what the case tests.  tests/test_gpu_mattn.py's mask allows almost every pair, its logits stay below
10 and its grids never take the workgroup remap in the backward; here:

  mask kind   what it is                                     the kernel lines it exists for
  ---------   --------------------------------------------   -----------------------------------------------------------------
  diag        only (i, i)                                     `p = masked ? 0 : __expf(s*scale - lse)` with lse == the one logit:
                                                              out == v and dV == dout bit for bit, dQ = dK = 0; every
                                                              off-diagonal tile skipped by `__ballot(mw != 0xffffffffu) == 0ull`
  blockdiag   tile(i) == tile(j)                              the ballot skip in the forward and in both backward phases with
                                                              the skipped tiles FIRST (query tiles > 0): `m` is still -inf when
                                                              the first computed tile arrives -> `alpha = mn == -INFINITY ? 1.f
                                                              : __expf(m - mn)` with m = -inf, mn finite
  anti        tile(i) + tile(j) == NT - 1                     the same with the one live tile anywhere in the walk, for tile 0
                                                              the (partial) last one: mask_word's `rem < 32` fill next to the skip
  sparse      ~5 scattered keys per row (+ the diagonal)      lanes of one wave disagree: a computed tile is fully blocked for
                                                              some lanes -> `mn == -INFINITY ? 1.f : ...` and `mn == -INFINITY ?
                                                              0.f : __expf(st - mn)` (exp(-inf - -inf) would be NaN), then the
                                                              first live tile of such a lane
  radius      cdist < 0.32 on normalised randn centres        the level-0 mask of the model: all of the above as production
                                                              meets them
  + padding   rows / columns >= n[b], n = T, T/2+1, 1, 33     `lse = 0` for dead rows, zero out / dQ / dK / dV rows, the skip of
                                                              whole dead query tiles and key tiles
  B = 4, H = 6: B * H * ny is a multiple of 8 for every shape -> the remapped branch of mattn_block in the forward AND the backward
  (a remap that ran one (head, tile block) twice and another never leaves a wrong slice behind); `sparse` at (512, 16) once more
  with B = 3: the plain branch.

Shapes: (T, hd) on the LDS limits of the backward, both sides of the T > 128 switch of waves per workgroup, a partial last tile,
one token.  Variants: `amp` -- q and k times 6, logits to about 240; `adv` -- the K / V rows of the padded keys hold 1e3 * sign(mean
query) and 1e4, so every blocked logit dwarfs every allowed one, and the result must be that of those rows zeroed.

Bars (mattn_ref.BARS) are tests/test_gpu_mattn.py's, but applied per row / per (cloud, head, part) slice: 1e-5 (f32), 2e-2 out and
3e-2 gradients (bf16), lse 1e-5 * max(1, |ref|) (f32) and 1e-2 absolute (bf16).  tests/test_mattn_ref_cpu.py shows that the
rounding of each mode alone (mattn_ref.restate_f32 / emulate_bf16 against fp64) stays within half of them -- except in `amp`:
there fp32 itself holds a logit of 240 to 9e-5 only (restate_f32: out up to 1.6e-5, lse 1.6e-5, dV 7e-6, dQ / dK 6.3e-5), and
the bf16 rounding of dS reaches 0.27 of a slice's dQ / dK where most rows are saturated.  So in `amp` every bar is max(bar, 3 x
the restatement's own error, from tests/golden/mattn_sparse_bars.json): measured on the CPU, never taken from a kernel.

Found by this file: the fp32 kernels formed `s * scale - m` as one fma, so the largest logit did not give exp(0) at head_dim 32
(scale is no power of two) and `diag` returned v off by one ulp; the kernels now round the product first, as the pass that
takes the maximum does (contraction off in the two fp32 kernels)."""
import json

import pytest
import torch

from tests import mattn_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    with open(R.TABLE) as f:
        return json.load(f)


def _run(c, qkv, dout, bits):
    """-> (out, lse, dqkv) of the kernels: out / dqkv through the autograd node, lse by calling the forward as ops.py does."""
    from gm3d_amd import ops
    from gm3d_amd._capi import check, lib
    scale = c.hd ** -0.5
    x = qkv.clone().requires_grad_(True)
    out = ops.attention_masked(x, bits, R.H, scale)
    out.backward(dout)
    out2 = torch.empty_like(out)
    lse = torch.empty(c.B, R.H, c.T, dtype=torch.float32, device="cuda")
    check(lib.gm3d_attention_masked_fwd(ops._ptr(qkv), ops._ptr(bits), ops._ptr(out2), ops._ptr(lse), c.B, c.T, R.H, c.hd, float(scale),
                                        ops._DT[qkv.dtype], ops._stream()), "gm3d_attention_masked_fwd")
    assert torch.equal(out2, out.detach())
    return out.detach(), lse, x.grad


@pytest.mark.parametrize("c", R.cases(), ids=R.case_id)
def test_masked_attention_against_fp64(c, table):
    from gm3d_amd import ops
    qkv, dout, mask, clean = (t.cuda() for t in R.inputs(c))
    assert torch.equal(mask, mask.transpose(1, 2))
    bits = ops.pack_mask(mask)
    scale = c.hd ** -0.5
    q64, d64 = clean.double(), dout.double()
    ref = R.reference_grad(q64, mask, R.H, c.hd, scale, d64)
    got = _run(c, qkv, dout, bits)
    assert all(bool(torch.isfinite(t).all()) for t in got), "non-finite output"
    err = R.errors(got, ref, q64, d64, mask, R.H, c.hd, c.dtype)
    bar = R.bars(c, table[R.case_id(c)])
    print("\nMATTN %s %s" % (R.case_id(c), " ".join("%s=%.3e/%.1e" % (k, err[k], bar[k]) for k in sorted(err))))
    out, lse, grad = got
    assert R.dead_rows_are_zero(out, lse, grad, mask, R.H, c.hd), "a row without an allowed key must give exact zeros"
    if c.kind == "diag" or c.T == 1:                      # one allowed key per live row: nothing to round
        live = ~mask.all(dim=2)
        v = qkv.view(c.B, c.T, 3, R.H * c.hd)[:, :, 2]
        dv = grad.view(c.B, c.T, 3, R.H * c.hd)[:, :, 2]
        assert torch.equal(out[live], v[live]), "diag: out must be the row's own v, bit for bit"
        assert torch.equal(dv[live], dout[live]), "diag: dV must be dout, bit for bit"
        assert "dq_zero" in err and "dk_zero" in err
    for k in sorted(err):
        assert err[k] <= bar[k], (R.case_id(c), k, err[k], bar[k])

"""-m gpu: the streaming attention kernels for 513 <= T <= 2048 (gm3d_amd/csrc/attention_long.hip, through ops.attention_masked; lse
through gm3d_attention_long_fwd) against the fp64 reference of tests/mattn_ref.py.  Cases, shapes and the bar rule:
tests/attention_long_cases.py; the bars come from tests/golden/attention_long_bars.json (measured on the CPU, never from a kernel).

  kind        what it is for in a kernel that walks the keys in 64-row chunks with a running maximum and sum
  ---------   ----------------------------------------------------------------------------------------------------------------
  none        no mask (bits = None): every tile computed, the rescale at every step; keys >= T blocked by mask_word alone
  blockdiag   whole key tiles blocked for most query tiles: the ballot skip, m still -inf when the first live tile arrives
  anti        the first allowed key of a row arrives only in a late chunk (for tile 0: in the ragged last one)
  sparse      lanes of one wave disagree: a computed tile is fully blocked for some lanes (alpha = 1, p = 0, no exp(-inf - -inf))
  radius      the model's mask
  + padding   clouds of T, T//2 + 1, 1 and 33 tokens: dead rows (zero out / lse / gradients), dead chunks
  amp / adv   logits to about 240 through the rescale; blocked keys whose logits and values dwarf the allowed ones must add nothing

Per case: errors within the bars for out, lse, dQ, dK, dV; dead rows exactly zero; a second forward + backward equal to the first bit
for bit.  One blockdiag case again under tests/poison.py (NaN, +inf, -inf): same bits.  Routing: ops.attention, the fused Point-MAE
stack (fused.py) and the Point-M2AE stack node (masked_stack.py) reach the new entry points above 512 tokens."""
import json
from contextlib import nullcontext

import pytest
import torch

from tests import attention_long_cases as C
from tests import mattn_ref as R
from tests import clouds, poison

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    with open(C.TABLE) as f:
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
    check(lib.gm3d_attention_long_fwd(ops._ptr(qkv), ops._ptr(bits), ops._ptr(out2), ops._ptr(lse), c.B, c.T, R.H, c.hd, float(scale),
                                      ops._DT[qkv.dtype], ops._stream()), "gm3d_attention_long_fwd")
    assert torch.equal(out2, out.detach())
    return out.detach(), lse, x.grad


def _gpu_inputs(c):
    from gm3d_amd import ops
    qkv, dout, mask, clean = (t.cuda() for t in C.inputs(c))
    assert torch.equal(mask, mask.transpose(1, 2))
    bits = None if c.kind == "none" else ops.pack_mask(mask)
    return qkv, dout, mask, clean, bits


@pytest.mark.parametrize("c", C.cases(), ids=C.case_id)
def test_long_attention_against_fp64(c, table):
    qkv, dout, mask, clean, bits = _gpu_inputs(c)
    ref = C.reference(c, clean, dout, mask)
    got = _run(c, qkv, dout, bits)
    assert all(bool(torch.isfinite(t).all()) for t in got), "non-finite output"
    err = R.errors(got, ref, clean.double(), dout.double(), mask, R.H, c.hd, c.dtype)
    bar = C.bars(c, table[C.case_id(c)])
    print("\nLATTN %s %s" % (C.case_id(c), " ".join("%s=%.3e/%.1e" % (k, err[k], bar[k]) for k in sorted(err))))
    out, lse, grad = got
    assert R.dead_rows_are_zero(out, lse, grad, mask, R.H, c.hd), "a row without an allowed key must give exact zeros"
    again = _run(c, qkv, dout, bits)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two runs must give the same bits"
    for k in sorted(err):
        assert err[k] <= bar[k], (C.case_id(c), k, err[k], bar[k])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blockdiag_under_poison(dtype):
    """No output element may depend on unwritten memory: out, lse and dqkv come from torch.empty / empty_like."""
    c = R.Case("base", "blockdiag", 577, 32, 4, dtype)
    qkv, dout, mask, clean, bits = _gpu_inputs(c)
    plain = _run(c, qkv, dout, bits)
    for pattern in ("nan", "+inf", "-inf"):
        with poison.poisoned(pattern) as state:
            got = _run(c, qkv, dout, bits)
        assert state.count >= 3, "out, lse and dqkv were not allocated under poison"
        poison.assert_same(plain, got, "attention_long[%s,%s]" % (dtype, pattern))


def test_attention_routes_to_the_long_kernels():
    """ops.attention (the Point-MAE models' entry) at 513 tokens == ops.attention_masked without a mask, bit for bit, backward
    included."""
    from gm3d_amd import ops
    g = torch.Generator().manual_seed(5)
    for dt in (torch.bfloat16, torch.float32):
        qkv = torch.randn(2, 513, 3 * 6 * 64, generator=g).to(dt).cuda()
        dout = torch.randn(2, 513, 6 * 64, generator=g).to(dt).cuda()
        res = []
        for fn in (lambda x: ops.attention(x, 6, 0.125), lambda x: ops.attention_masked(x, None, 6, 0.125)):
            x = qkv.clone().requires_grad_(True)
            out = fn(x)
            out.backward(dout)
            res.append((out.detach(), x.grad))
        assert bool(torch.isfinite(res[0][0]).all()) and bool(res[0][0].any())
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-12)


def test_fused_stack_equals_per_op_path_at_513_tokens(monkeypatch):
    """A two-block Point-MAE TransformerEncoder at 513 tokens: the fused stack (fused.py) against the per-op modules
    (ops.attention), bf16, within the bf16 bars of mattn_ref (out 2e-2, gradients 3e-2)."""
    from gm3d_amd import models_mae_learn_loss as M
    torch.manual_seed(0)
    enc = M.TransformerEncoder(embed_dim=384, depth=2, num_heads=6, drop_path_rate=[0.0, 0.0]).cuda().train()
    norm = torch.nn.LayerNorm(384).cuda()
    x = torch.randn(2, 513, 384, device="cuda")
    pos = torch.randn(2, 513, 384, device="cuda") * 0.3
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(M, "FUSED_STACK", fused)
        xi = x.clone().requires_grad_(True)
        for p in enc.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = enc(xi, pos, norm=norm)
        (out.float() * torch.linspace(0.5, 1.5, 384, device="cuda")).sum().backward()
        res[fused] = (out.detach().float(), xi.grad.clone(), enc.blocks[0].attn.qkv.weight.grad.detach().clone())
    assert bool(torch.isfinite(res[True][0]).all())
    assert _rel(res[True][0], res[False][0]) <= R.BARS["bf16"]["out"]
    assert _rel(res[True][1], res[False][1]) <= R.BARS["bf16"]["dq"]
    assert _rel(res[True][2], res[False][2]) <= R.BARS["bf16"]["dq"]


@pytest.mark.parametrize("bf16", [True, False])
def test_masked_stack_equals_per_op_path_at_640_tokens(bf16):
    """A two-block Point-M2AE BlockStack at G = 640 under a radius mask from ops.radius_mask_bits: the stack node (masked_stack.py)
    against the per-op nodes (ops.attention_masked).  The forward kernels are the same in the same order: outputs equal; gradients
    within the bf16 bar (3e-2) / the fp32 summation-order band of tests/test_gpu_masked_stack.py (2e-5)."""
    from gm3d_amd import ops
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    B, T, Cw = 2, 640, 96
    stack = P.BlockStack(Cw, 2, 6, [0.0, 0.0]).cuda().train()
    x = torch.randn(B, T, Cw, device="cuda")
    pos = torch.randn(B, T, Cw, device="cuda") * 0.3
    cen = clouds.pc_norm(torch.randn(B, T, 3)).cuda()
    vis = torch.rand(B, T, device="cuda") < 0.7
    bits = ops.radius_mask_bits(cen, vis, 0.32)
    keep = vis.unsqueeze(-1).float()
    res = {}
    was = P.STACK_NODE
    try:
        for node in (True, False):
            P.STACK_NODE = node
            xi = x.clone().requires_grad_(True)
            for p in stack.parameters():
                p.grad = None
            with (torch.autocast("cuda", dtype=torch.bfloat16) if bf16 else nullcontext()):
                out = stack(xi.bfloat16() if bf16 else xi, pos.bfloat16() if bf16 else pos, bits)
            (out.float() * keep * torch.linspace(0.5, 1.5, Cw, device="cuda")).sum().backward()
            res[node] = (out.detach().float() * keep, xi.grad.clone(), stack.blocks[0].attn.qkv.weight.grad.detach().clone())
    finally:
        P.STACK_NODE = was
    assert bool(torch.isfinite(res[True][0]).all()) and bool(res[True][0].any())
    assert torch.equal(res[True][0], res[False][0])
    tol = R.BARS["bf16"]["dq"] if bf16 else 2e-5
    assert _rel(res[True][1], res[False][1]) <= tol and _rel(res[True][2], res[False][2]) <= tol

"""-m gpu: attention WITHOUT a mask up to 512 tokens -- the whole-head kernels (gm3d_amd/csrc/attention.hip: T <= 128, head_dim 64), the
flash kernels with a null mask (csrc/attention_masked.hip) and the padded form (the streaming kernels at 513 rows, attention.fwd / bwd
with pad=True as fused.py calls them) -- against the fp64 reference of tests/mattn_ref.py, per row and per (cloud, head) slice.
Cases, inputs and the bar rule: tests/attention_plain_cases.py; the bars of the `amp` and `scale` cases come from
tests/golden/attention_plain_bars.json (measured on the CPU, never from a kernel).  The route of a case is read from attention.route
and shown in its id; it is not asserted here (tests/golden/attention_routes.json pins the routes).

Per case: out, lse and dqkv from attention.fwd / attention.bwd; for the head and flash routes the same bits from ops.attention /
ops.attention_masked(x, None, ...) through autograd; everything finite; every metric of mattn_ref.errors within its bar; a second
forward + backward equal to the first bit for bit.  Padded form: the lse has the shape fwd documents, its rows beyond T are ignored.
T = 1 (scale 0.125 and 0.11): out == v and dV == dout bit for bit, dQ and dK under the dq_zero / dk_zero bars.

What this is for: a whole-tensor bar averages one wrong (cloud, head) tile away (tests/parity.py).  A kernel that skipped the
`key < T` guard of one tile, dropped the subtraction of the row maximum or zeroed one (cloud, head) slice fails here.

Measured (MI355X), worst error / bar over a route's cases: head 0.62 (dQ, bf16 `amp` T = 64; base cases 0.42 at most in bf16, 0.24 in
fp32), flash 0.34, padded 0.34 -- all three at `amp`, where the bar is 3 x the restatement and the kernels sit at the restatement.
Found by the `scale` cases: the whole-head backward fused `s * scale - lse` into one fma, so at scale 0.11 and T = 1 the fp32 dV was
dout * exp(+-1e-7) (dv = 1.1e-7 where the identity demands equality); fixed in csrc/attention.hip (contract(off) where a logit is formed).
"""
import json

import pytest
import torch

from tests import attention_plain_cases as C
from tests import mattn_ref as R

pytestmark = pytest.mark.gpu


def _route_name(c):
    from gm3d_amd import attention
    dt, pad = R.DTYPES[c.dtype], c.call == "pad"
    f = attention.route(c.T, c.hd, dt, False, False, head=True, pad=pad)
    if c.call == "pad":
        return "padded(%s%d+%s%d)" % (f + attention.route(c.T, c.hd, dt, False, True, head=True, pad=True))
    return f[0]


def _id(c):
    return "%s-%s" % (_route_name(c), C.case_id(c))


@pytest.fixture(scope="module")
def table():
    with open(C.TABLE) as f:
        return json.load(f)


def _run(c, qkv, dout):
    """-> (out (B,T,H*hd), lse (B,H,T), dqkv (B,T,3*H*hd) | None) from attention.fwd / attention.bwd, as the stacks call them"""
    from gm3d_amd import attention
    B, T, hd, pad = c.B, c.T, c.hd, c.call == "pad"
    scale = C.scale_of(c)
    q2, d2 = qkv.view(B * T, -1), dout.view(B * T, -1)
    out, lse = attention.fwd(q2, None, B, T, C.H, hd, scale, head=True, pad=pad)
    rows = attention.route(T, hd, qkv.dtype, False, False, head=True, pad=pad)[1]
    assert tuple(out.shape) == (B * T, C.H * hd) and out.dtype == qkv.dtype
    assert tuple(lse.shape) == (B, C.H, rows) and lse.dtype == torch.float32, "lse must be (B,H,T), (B,H,PAD_T) from the padded form"
    dqkv = None
    if c.call != "fwd":
        dqkv = attention.bwd(q2, None, out, d2, lse, B, T, C.H, hd, scale, head=True, pad=pad)
        assert tuple(dqkv.shape) == tuple(q2.shape) and dqkv.dtype == qkv.dtype
        dqkv = dqkv.view(B, T, -1)
    return out.view(B, T, -1), lse[:, :, :T].contiguous(), dqkv


def _through_autograd(c, fn, qkv, dout):
    x = qkv.clone().requires_grad_(c.call != "fwd")
    out = fn(x, C.H, C.scale_of(c))
    if c.call == "fwd":
        return out.detach(), None
    out.backward(dout)
    return out.detach(), x.grad


@pytest.mark.parametrize("c", C.cases(), ids=_id)
def test_plain_attention_against_fp64(c, table):
    from gm3d_amd import ops
    qkv, dout, mask = (t.cuda() for t in C.inputs(c))
    ref = C.reference(c, qkv, dout, mask)
    out, lse, grad = _run(c, qkv, dout)
    got = (out, lse, grad if grad is not None else torch.zeros_like(qkv))
    for name, t in zip(("out", "lse", "dqkv"), got):
        assert bool(torch.isfinite(t).all()), (_id(c), name, "non-finite")
    err = C.errors(c, got, ref, qkv, dout, mask)
    bar = C.bars(c, table[C.case_id(c)])
    print("\nPATTN %s %s" % (_id(c), " ".join("%s=%.3e/%.1e" % (k, err[k], bar[k]) for k in sorted(err))))

    route = _route_name(c)
    if route in ("head", "flash"):
        fns = [("ops.attention", ops.attention)] if route == "head" or c.hd == 64 else []
        if route == "flash":
            fns.append(("ops.attention_masked", lambda x, H, s: ops.attention_masked(x, None, H, s)))
        for name, fn in fns:
            o, g = _through_autograd(c, fn, qkv, dout)
            assert torch.equal(o, out), (_id(c), name, "out differs from attention.fwd")
            assert g is None or torch.equal(g, grad), (_id(c), name, "dqkv differs from attention.bwd")

    again = _run(c, qkv, dout)
    for name, a, b in zip(("out", "lse", "dqkv"), (out, lse, grad), again):
        assert a is None or torch.equal(a, b), (_id(c), name, "two runs must give the same bits")

    if c.T == 1:
        B, hd = c.B, c.hd
        assert torch.equal(out.view(B, C.H, hd), qkv.view(B, 3, C.H, hd)[:, 2]), (_id(c), "one key: out must be v bit for bit")
        assert torch.equal(grad.view(B, 3, C.H * hd)[:, 2], dout.view(B, C.H * hd)), (_id(c), "one key: dV must be dout bit for bit")
        assert "dq_zero" in err and "dk_zero" in err

    for k in sorted(err):
        if not err[k] <= bar[k]:
            e, where = C.locate(c, k, got, ref, qkv, dout)
            pytest.fail("%s %s: %.3e over the bar %.1e, worst at %s" % (_id(c), k, e, bar[k], where))

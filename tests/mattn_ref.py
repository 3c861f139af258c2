"""Plain-torch side of the masked-attention tests (tests/test_mattn_ref_cpu.py, tests/test_gpu_mattn_sparse.py): the mask
structures, the inputs of every case, an fp64 reference, two restatements whose own distance from fp64 is what the bars are measured
against (`emulate_bf16`: the rounding points of the bf16 kernels; `restate_f32`: the same attention in torch fp32), and the
metrics.  Nothing here imports the package under test; every function runs on the CPU and, given GPU tensors, on the GPU.

Inputs are always drawn on the CPU from a seeded generator, so the table in tests/golden/mattn_sparse_bars.json (written from this
file on the CPU) is about exactly the tensors the GPU test feeds the kernels."""
import collections
import math
import os

import torch

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mattn_sparse_bars.json")

H = 6
KINDS = ("diag", "blockdiag", "anti", "sparse", "radius")
SHAPES = ((512, 16), (480, 32), (256, 64), (129, 32), (128, 32), (97, 64), (33, 16), (1, 32))
LARGE_KINDS = ("blockdiag", "sparse", "radius")
LARGE_SHAPES = ((512, 16), (256, 64), (97, 64))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}

# tol: `out` per live row, relative to the largest allowed |v| of the row (tests/test_gpu_mattn.py's 1e-5 / 2e-2);
# lse: relative to max(1, |ref|) in fp32, absolute in bf16; grad: per (cloud, head, part) slice (1e-5 / 3e-2, same file);
# zero: |dQ|, |dK| relative to max |dout| where the true gradient is identically zero (one allowed key per row)
BARS = {"f32": {"out": 1e-5, "lse": 1e-5, "dq": 1e-5, "dk": 1e-5, "dv": 1e-5, "dq_zero": 1e-5, "dk_zero": 1e-5},
        "bf16": {"out": 2e-2, "lse": 1e-2, "dq": 3e-2, "dk": 3e-2, "dv": 3e-2, "dq_zero": 1e-5, "dk_zero": 1e-5}}

Case = collections.namedtuple("Case", "variant kind T hd B dtype")


def case_id(c):
    return "%s-%s-T%d-hd%d-B%d-%s" % c


def cases():
    """base: every kind x shape x dtype at B = 4 (B * H * ny is a multiple of 8: the workgroup remap is taken), `anti` left out
    at T = 1 (dead rows only), and `sparse` once more at B = 3 (remap not taken).  amp / adv: the large-logit variants."""
    out = []
    for dt in DTYPES:
        for kind in KINDS:
            for T, hd in SHAPES:
                if not (kind == "anti" and T == 1):
                    out.append(Case("base", kind, T, hd, 4, dt))
        out.append(Case("base", "sparse", 512, 16, 3, dt))
        for variant in ("amp", "adv"):
            for kind in LARGE_KINDS:
                for T, hd in LARGE_SHAPES:
                    out.append(Case(variant, kind, T, hd, 4, dt))
    return out


def bars(c, measured=None):
    """The bars of case `c`.  amp: every bar is max(bar, 3 x the restatement's own error) -- `measured` is the case's row of
    mattn_sparse_bars.json ("as close to fp64 as the restatement is, x3", the convention of tests/test_gpu_m2ae.py).  For bf16
    this moves dQ / dK only; in fp32 the format itself holds a logit of 240 to 9e-5, which restate_f32 shows in out, lse and dV
    as well (tests/test_mattn_ref_cpu.py)."""
    b = dict(BARS[c.dtype])
    if c.variant == "amp":
        for k in measured:
            b[k] = max(b[k], 3.0 * measured[k])
    return b


# ------------------------------------------------------------------------------------------------------------------ masks
def masks(kind, B, T, seed):
    """(B,T,T) bool, True = blocked, symmetric.  tile(i) = i // 32, NT = ceil(T / 32)."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(T)
    tile, NT = i // 32, (T + 31) // 32
    if kind == "diag":
        allowed = (i[:, None] == i[None, :]).expand(B, T, T)
    elif kind == "blockdiag":
        allowed = (tile[:, None] == tile[None, :]).expand(B, T, T)
    elif kind == "anti":
        allowed = (tile[:, None] + tile[None, :] == NT - 1).expand(B, T, T)
    elif kind == "sparse":
        u = torch.rand(B, T, T, generator=g) < 4.0 / T
        allowed = u | u.transpose(1, 2) | torch.eye(T, dtype=torch.bool)
    elif kind == "radius":
        c = torch.randn(B, T, 3, generator=g, dtype=torch.float64)
        c = c / c.norm(dim=-1).amax(dim=1)[:, None, None]
        d = c[:, :, None, :] - c[:, None, :, :]                     # (a - b)^2 == (b - a)^2 bit for bit: exactly symmetric
        allowed = (d * d).sum(-1) < 0.32 ** 2
    else:
        raise ValueError(kind)
    return ~allowed.clone()


def pad_lengths(B, T):
    return [T, T // 2 + 1, 1, min(33, T)][:B]


def pad(mask, n):
    """Block every row and column at or beyond n[b] of cloud b."""
    T = mask.shape[1]
    valid = torch.arange(T, device=mask.device)[None, :] < torch.as_tensor(n, device=mask.device)[:, None]
    return mask | ~valid[:, None, :] | ~valid[:, :, None]


def seed_of(c):
    return 1000 * KINDS.index(c.kind) + 7 * c.T + c.hd + c.B


def inputs(c):
    """-> (qkv, dout, mask, qkv_clean) on the CPU; qkv / dout in the case's dtype (bf16: what the reference sees is the rounded
    value).  qkv_clean is what the reference is computed from: qkv itself, except in `adv`, where the K and V rows of the padded
    keys -- 1e3 * sign(mean query) per head and 1e4 in qkv, so that every blocked logit and value dwarfs every allowed one --
    are zero: a blocked pair contributes exactly nothing."""
    dtype = DTYPES[c.dtype]
    n = pad_lengths(c.B, c.T)
    mask = pad(masks(c.kind, c.B, c.T, seed_of(c)), n)
    g = torch.Generator().manual_seed(seed_of(c) + 1)
    x = (torch.randn(c.B, c.T, 3, H, c.hd, generator=g) * 1.2)
    dout = torch.randn(c.B, c.T, H * c.hd, generator=g).to(dtype)
    if c.variant == "amp":
        x[:, :, :2] *= 6.0
    clean = x
    if c.variant == "adv":
        clean = x.clone()
        sgn = torch.sign(x[:, :, 0].mean(dim=1))                     # (B,H,hd)
        for b in range(c.B):
            x[b, n[b]:, 1] = 1e3 * sgn[b]
            x[b, n[b]:, 2] = 1e4
            clean[b, n[b]:, 1:] = 0.0
    shape = (c.B, c.T, 3 * H * c.hd)
    return x.reshape(shape).to(dtype), dout, mask, clean.reshape(shape).to(dtype)


# ------------------------------------------------------------------------------------------------- reference, restatements
def _heads(x, parts, hd):
    B, T, _ = x.shape
    return x.reshape(B, T, parts, -1, hd).permute(2, 0, 3, 1, 4)     # (parts, B, H, T, hd)


def _attention(qkv, mask, H, hd, scale):
    """softmax((q k^T) * scale, blocked pairs removed) v on the (B,T,3,H,hd) layout, in qkv's own precision (the formula of
    tests/test_gpu_mattn.py::_ref) -> out (B,T,H*hd), lse (B,H,T): logsumexp over the allowed keys, 0 for a row without one."""
    B, T, _ = qkv.shape
    q, k, v = _heads(qkv, 3, hd)
    s = (q @ k.transpose(-2, -1)) * scale
    s = s.masked_fill(mask.unsqueeze(1), float("-inf"))
    p = torch.nan_to_num(s.softmax(dim=-1), nan=0.0)                 # a row with no allowed key: zeros
    out = (p @ v).transpose(1, 2).reshape(B, T, H * hd)
    dead = mask.all(dim=2).unsqueeze(1)
    lse = torch.logsumexp(s.detach().masked_fill(dead.unsqueeze(-1), 0.0), dim=-1).masked_fill(dead, 0.0)
    return out, lse


def reference(qkv64, mask, H, hd, scale):
    assert qkv64.dtype == torch.float64
    return _attention(qkv64, mask, H, hd, scale)


def _with_grad(qkv, mask, H, hd, scale, dout):
    x = qkv.detach().clone().requires_grad_(True)
    out, lse = _attention(x, mask, H, hd, scale)
    out.backward(dout)
    return out.detach(), lse, x.grad


def reference_grad(qkv64, mask, H, hd, scale, dout64):
    """-> (out, lse, dqkv) in fp64, the gradient by autograd."""
    assert qkv64.dtype == torch.float64 and dout64.dtype == torch.float64
    return _with_grad(qkv64, mask, H, hd, scale, dout64)


def _bf(x):
    return x.bfloat16().float()


def _flash(qkv, mask, H, hd, scale, dout, rnd):
    """The operator as its interface defines it -- the forward keeps out and lse, not P; the backward recomputes P = exp(s - lse)
    and takes delta = <dO, out> -- on whole matrices in fp32, `rnd` applied where the bf16 kernels round (identity: plain fp32).
    No tiles, no running maximum, no skipping: those must not change the result beyond this rounding."""
    B, T, _ = qkv.shape
    q, k, v = _heads(rnd(qkv.float()), 3, hd)
    blocked = mask.unsqueeze(1)
    s = ((q @ k.transpose(-2, -1)) * scale).masked_fill(blocked, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    dead = m == float("-inf")
    e = torch.exp(s - m.masked_fill(dead, 0.0))                      # blocked: exp(-inf) = 0
    l = e.sum(dim=-1, keepdim=True)
    o = rnd((rnd(e) @ v) / l.masked_fill(dead, 1.0))
    lse = (m + torch.log(l.masked_fill(dead, 1.0))).masked_fill(dead, 0.0)
    do, = _heads(rnd(dout.float()), 1, hd)
    # dP = dO V^T and delta = <dO, out> from ONE product, so both are summed in the same order, as any implementation's dot
    # product routine would: a row with one allowed key (out == v) then has dP - delta == 0 exactly
    dpo = do @ torch.cat([v, o], dim=-2).transpose(-2, -1)            # (B,H,T,2T)
    delta = dpo[..., T:].diagonal(dim1=-2, dim2=-1).unsqueeze(-1)
    p = torch.exp(s - lse)
    ds = rnd(p * (dpo[..., :T] - delta) * scale)
    dv = rnd(rnd(p).transpose(-2, -1) @ do)
    dq, dk = rnd(ds @ k), rnd(ds.transpose(-2, -1) @ q)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B, T, 3 * H * hd)
    return o.permute(0, 2, 1, 3).reshape(B, T, H * hd), lse.squeeze(-1), dqkv


def restate_f32(qkv, mask, H, hd, scale, dout):
    """The same attention in torch fp32 -> (out, lse, dqkv): what fp32 arithmetic gives for this operator.  The backward is the
    one the interface implies (P from the saved lse, delta from out), not autograd's softmax backward, which keeps P and forms
    sum_k P_k dP_k from it.  The two agree to 1e-6 at the usual logits; at logits of 240 (`amp`), where most rows are
    saturated and dP - delta cancels, this form loses up to 6.3e-5 of a slice's dQ / dK and autograd's 1.1e-5 .. 2.4e-5 (measured
    on the CPU) -- a property of the formulation in fp32, so it belongs in the yardstick."""
    return _flash(qkv, mask, H, hd, scale, dout, lambda x: x)


def emulate_bf16(qkv, mask, H, hd, scale, dout):
    """Where the bf16 kernels round -> (out, lse, dqkv) as fp32 tensors holding bf16 values.  Forward: fp32 logits from the bf16
    inputs, exp(s - rowmax) summed in fp32 but rounded to bf16 as the operand of P.V, the quotient rounded to bf16.  Backward:
    delta = <dO, rounded out>; P = exp(s - lse) and dS * scale = P (dP - delta) scale rounded to bf16 before dV = P^T dO,
    dQ = dS K, dK = dS^T Q; the three gradients rounded to bf16."""
    return _flash(qkv, mask, H, hd, scale, dout, _bf)


# ---------------------------------------------------------------------------------------------------------------- metrics
def errors(got, ref, qkv64, dout64, mask, H, hd, dtype):
    """got, ref = (out, lse, dqkv) -> {metric: error}, each the largest ratio the assertion of that metric bounds:
    out   per live row and head: |out - ref| / max over the row's ALLOWED keys j of |v_j| (the scale of a convex combination);
    lse   per live row: |lse - ref| / max(1, |ref|) for f32, |lse - ref| for bf16;
    dq, dk, dv   per (cloud, head): max |g - gref| / max(max |gref| of the slice, 1e-2 * max |gref| of the part);
    dq_zero, dk_zero   instead of dq / dk where gref of the whole part is identically zero (every live row has ONE allowed key:
    `diag`, T = 1): max |g| / max |dout|."""
    out, lse, grad = (t.double() for t in got)
    rout, rlse, rgrad = ref
    B, T, _ = qkv64.shape
    live = ~mask.all(dim=2)                                           # (B,T)
    vmax = _heads(qkv64, 3, hd)[2].abs().amax(dim=-1)                  # (B,H,T)
    row_scale = vmax.unsqueeze(2).masked_fill(mask.unsqueeze(1), 0.0).amax(dim=-1)       # (B,H,T): max over allowed keys
    eo = _heads(out - rout, 1, hd)[0].abs().amax(dim=-1)              # (B,H,T)
    lv = live.unsqueeze(1).expand_as(eo)
    res = {"out": float((eo[lv] / row_scale[lv]).max())}
    el = (lse - rlse).abs()
    if dtype == "f32":
        el = el / rlse.abs().clamp_min(1.0)
    res["lse"] = float(el[lv].max())
    eg = _heads(grad - rgrad, 3, hd).abs().amax(dim=(-2, -1))          # (3,B,H)
    sg = _heads(rgrad, 3, hd).abs().amax(dim=(-2, -1))
    for i, name in enumerate(("dq", "dk", "dv")):
        part = float(sg[i].max())
        if part == 0.0:
            res[name + "_zero"] = float(eg[i].max() / dout64.abs().max())
        else:
            res[name] = float((eg[i] / sg[i].clamp_min(1e-2 * part)).max())
    return res


def dead_rows_are_zero(out, lse, grad, mask, H, hd):
    """A query without an allowed key: out, lse and its rows of dQ, dK, dV are exactly 0."""
    dead = mask.all(dim=2)
    return (not bool(out[dead].any()) and not bool(grad[dead].any())
            and not bool(lse[dead.unsqueeze(1).expand_as(lse)].any()))


def worst(table, ids, bar_of):
    """{metric: (largest error / bar, case id)} over the cases `ids` of a {case id: {metric: error}} table."""
    w = {}
    for cid in ids:
        for k, e in table[cid].items():
            r = e / bar_of(cid)[k]
            if k not in w or r > w[k][0]:
                w[k] = (r, cid)
    return w


def tile_structure(mask_b):
    """(T,T) bool -> (blocked, NT): blocked[i, kt] = every key of key tile kt is blocked for row i (keys >= T count as
    blocked, as the kernels force them)."""
    T = mask_b.shape[0]
    NT = int(math.ceil(T / 32))
    m = torch.ones(T, 32 * NT, dtype=torch.bool)
    m[:, :T] = mask_b
    return m.view(T, NT, 32).all(dim=-1), NT

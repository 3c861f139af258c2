"""The cases of the unmasked-attention tests (T <= 512, bits = None), shared by tests/golden/make_attention_plain_bars.py (CPU: writes
the bars table), tests/test_attention_plain_cpu.py and tests/test_gpu_attention_plain.py.  Everything numerical comes from
tests/mattn_ref.py; this file only names the cases, draws their inputs by mattn_ref.inputs' recipe without a mask, states the bar rule
and, for a failure message, finds where a metric of mattn_ref.errors is worst.  Nothing here imports the package under test.

Every case has kind `none`: no mask for the kernels, an all-false mask for the reference; no padding, no dead rows.  H = 6.  Three
routes (gm3d_amd/attention.py names the one a case takes; the case id of the GPU test shows it):

  head     gm3d_attention_fwd / _bwd (csrc/attention.hip), head_dim 64, T <= 128.  T = 1, 31, 32, 33, 64, 65, 96, 97, 128 in both
           dtypes: every NT (bf16: 1..4 tiles) and MT (fp32: 2, 4) instantiation on both sides of each switch; `amp` at 33, 64, 97,
           128; `scale` (0.11, no power of two: `s * scale` rounds) at 1, 33, 128; B = 43 at T = 64 (258 workgroups: more than one
           per CU); B = 3 at T = 97
  flash    gm3d_attention_masked_fwd / _bwd with a null mask (csrc/attention_masked.hip), 129 <= T <= 512, head_dim 16, 32, 64.  In
           bf16 at head_dim 64 the backward holds 256 tokens, so (257, 64) and (480, 64) run the forward only (`call` = "fwd")
  padded   attention.fwd / bwd(head=True, pad=True) as fused.py calls them: bf16, head_dim 64, T = 257, 480 (flash forward, its lse
           padded, padded backward), 481, 512 (both padded, on the streaming kernels at 513 rows)

Variants: `base`; `amp` (q and k times 6: logits to about 240, through -INFINITY and exp(s - m)); `scale`.  The scale of a case is
head_dim ** -0.5, and 0.11 in `scale`.

Bars: base cases mattn_ref.BARS as they stand, and tests/test_attention_plain_cpu.py demands that the restatement of every base case
stays within HALF of each; `amp` and `scale` max(bar, 3 x the restatement's own distance from fp64), the distance measured on the CPU
by `measure` and committed in tests/golden/attention_plain_bars.json.  No bar is ever derived from a kernel's output.  (T = 31 is no
`amp` length: the bf16 restatement alone is 7.7e-2 off in dQ / dK there.)"""
import collections
import os

import torch

from tests import mattn_ref as R

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_plain_bars.json")

H = R.H
SCALE = 0.11
VARIANTS = ("base", "amp", "scale")
CALLS = ("full", "fwd", "pad")          # forward + backward | forward only | forward + backward with pad=True

HEAD_T = (1, 31, 32, 33, 64, 65, 96, 97, 128)
HEAD_AMP_T = (33, 64, 97, 128)
HEAD_SCALE_T = (1, 33, 128)
FLASH_F32 = ((129, 64), (256, 64), (257, 64), (512, 64), (129, 32), (480, 32), (512, 16))
FLASH_BF16 = ((129, 64), (256, 64), (480, 32), (512, 16))
FLASH_BF16_FWD = ((257, 64), (480, 64))
FLASH_AMP = ((256, 64), (512, 16))
PAD_LENGTHS = (257, 480, 481, 512)
PAD_AMP = (257, 512)

Case = collections.namedtuple("Case", "variant kind T hd B dtype call")


def case_id(c):
    return "%s-%s-T%d-hd%d-B%d-%s-%s" % c


def cases():
    out = []
    for dt in R.DTYPES:
        for T in HEAD_T:
            out.append(Case("base", "none", T, 64, 4, dt, "full"))
        out.append(Case("base", "none", 97, 64, 3, dt, "full"))
        out.append(Case("base", "none", 64, 64, 43, dt, "full"))
        for T in HEAD_AMP_T:
            out.append(Case("amp", "none", T, 64, 4, dt, "full"))
        for T in HEAD_SCALE_T:
            out.append(Case("scale", "none", T, 64, 4, dt, "full"))
        for T, hd in (FLASH_F32 if dt == "f32" else FLASH_BF16):
            out.append(Case("base", "none", T, hd, 4, dt, "full"))
        out.append(Case("base", "none", 129, 64, 3, dt, "full"))
        for T, hd in FLASH_AMP:
            out.append(Case("amp", "none", T, hd, 4, dt, "full"))
    for T, hd in FLASH_BF16_FWD:
        out.append(Case("base", "none", T, hd, 4, "bf16", "fwd"))
    for T in PAD_LENGTHS:
        out.append(Case("base", "none", T, 64, 4, "bf16", "pad"))
    out.append(Case("base", "none", 481, 64, 3, "bf16", "pad"))
    for T in PAD_AMP:
        out.append(Case("amp", "none", T, 64, 4, "bf16", "pad"))
    return out


def scale_of(c):
    return SCALE if c.variant == "scale" else c.hd ** -0.5


def metrics_of(c):
    """the metrics of mattn_ref.errors a case is held to.  T = 1: the true dQ and dK are identically zero"""
    if c.call == "fwd":
        return ["lse", "out"]
    return sorted(["lse", "out", "dv"] + (["dq_zero", "dk_zero"] if c.T == 1 else ["dq", "dk"]))


# Chosen on the CPU from the restatement alone: at logits of 240 most rows are saturated, and with most seeds one (cloud, head) slice of
# the T = 33 case has so small a true dQ / dK that emulate_bf16 itself is 7e-2 .. 1.6e-1 of it away, which would put that bar at
# 0.2 .. 0.5.  With this one every bf16 `amp` row stays within AMP_BF16_MAX in dQ / dK (tests/test_attention_plain_cpu.py).
SEED_SALT = 6 * 1000003
AMP_BF16_MAX = 2.6e-2


def seed_of(c):
    return SEED_SALT + 100000 * (1 + VARIANTS.index(c.variant)) + 20000 * CALLS.index(c.call) + 7 * c.T + c.hd + c.B


def inputs(c):
    """-> (qkv, dout, mask) on the CPU, by mattn_ref.inputs' recipe: a CPU generator seeded from the case, randn * 1.2, `amp`
    multiplies q and k by 6; qkv / dout in the case's dtype (bf16: what the reference sees is the rounded value).  mask: all false."""
    dtype = R.DTYPES[c.dtype]
    g = torch.Generator().manual_seed(seed_of(c))
    x = torch.randn(c.B, c.T, 3, H, c.hd, generator=g) * 1.2
    dout = torch.randn(c.B, c.T, H * c.hd, generator=g).to(dtype)
    if c.variant == "amp":
        x[:, :, :2] *= 6.0
    return x.reshape(c.B, c.T, 3 * H * c.hd).to(dtype), dout, torch.zeros(c.B, c.T, c.T, dtype=torch.bool)


def bars(c, measured):
    """`measured`: the case's row of attention_plain_bars.json"""
    b = {k: R.BARS[c.dtype][k] for k in metrics_of(c)}
    if c.variant != "base":
        for k in b:
            b[k] = max(b[k], 3.0 * measured[k])
    return b


def reference(c, qkv, dout, mask):
    """fp64 (out, lse, dqkv) of the case on qkv's device"""
    return R.reference_grad(qkv.double(), mask, H, c.hd, scale_of(c), dout.double())


def errors(c, got, ref, qkv, dout, mask):
    err = R.errors(got, ref, qkv.double(), dout.double(), mask, H, c.hd, c.dtype)
    return {k: err[k] for k in metrics_of(c)}


def measure(c):
    """CPU: the restatement of the case's mode (mattn_ref.restate_f32 / emulate_bf16) against fp64 -> {metric: error}.  One thread:
    the figures are those of one fixed summation order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        qkv, dout, mask = inputs(c)
        ref = reference(c, qkv, dout, mask)
        fn = R.emulate_bf16 if c.dtype == "bf16" else R.restate_f32
        got = fn(qkv, mask, H, c.hd, scale_of(c), dout)
        assert all(bool(torch.isfinite(t).all()) for t in got + ref), case_id(c)
        return errors(c, got, ref, qkv, dout, mask)
    finally:
        torch.set_num_threads(threads)


def locate(c, metric, got, ref, qkv, dout):
    """Where `metric` of mattn_ref.errors is worst, for an unmasked case -> (error, "where: got against ref").  out: the (cloud,
    head, row), lse: the (cloud, head, row), a gradient: the (cloud, head) slice; the two numbers are those of the element of that
    row or slice that is furthest off."""
    out, lse, grad = (t.double() for t in got)
    rout, rlse, rgrad = ref
    q64 = qkv.double()

    def at(t, idx):
        return tuple(int(i) for i in torch.unravel_index(torch.as_tensor(idx), t.shape))

    if metric == "out":
        vmax = R._heads(q64, 3, c.hd)[2].abs().amax(dim=(-2, -1), keepdim=True)         # every key is allowed: one scale per (b, h)
        g, r = R._heads(out, 1, c.hd)[0], R._heads(rout, 1, c.hd)[0]                    # (B,H,T,hd)
        e = (g - r).abs().amax(dim=-1) / vmax.squeeze(-1)
        b, h, t = at(e, e.argmax())
        d = int((g - r)[b, h, t].abs().argmax())
        return float(e[b, h, t]), "cloud %d head %d row %d col %d: %.9g against %.9g" % (b, h, t, d, g[b, h, t, d], r[b, h, t, d])
    if metric == "lse":
        e = (lse - rlse).abs()
        if c.dtype == "f32":
            e = e / rlse.abs().clamp_min(1.0)
        b, h, t = at(e, e.argmax())
        return float(e[b, h, t]), "cloud %d head %d row %d: %.9g against %.9g" % (b, h, t, lse[b, h, t], rlse[b, h, t])
    i = ("dq", "dk", "dv").index(metric[:2])
    g, r = R._heads(grad, 3, c.hd)[i], R._heads(rgrad, 3, c.hd)[i]                      # (B,H,T,hd)
    e = (g - r).abs().amax(dim=(-2, -1))
    if metric.endswith("_zero"):
        e = e / dout.double().abs().max()
    else:
        s = r.abs().amax(dim=(-2, -1))
        e = e / s.clamp_min(1e-2 * float(s.max()))
    b, h = at(e, e.argmax())
    t, d = at(g[b, h], (g - r)[b, h].abs().argmax())
    return float(e[b, h]), "cloud %d head %d (row %d col %d): %.9g against %.9g" % (b, h, t, d, g[b, h, t, d], r[b, h, t, d])

"""The cases of the long-attention tests (513 <= T <= 2048: gm3d_amd/csrc/attention_long.hip), shared by
tests/golden/make_attention_long_bars.py (CPU: writes the bars table), tests/test_attention_long_cpu.py and
tests/test_gpu_attention_long.py.  Everything numerical comes from tests/mattn_ref.py; this file only names the cases, adds the kind
`none` (no mask at all: bits = None for the kernel, an all-false mask for the reference) and states the bar rule.  Nothing here
imports the package under test.

Shapes (T, hd), with the streaming kernels' 64-row chunks, 32-row tiles and 256-query (forward) / 128-row (backward) workgroups:
  (513, 64), (513, 16)   one row and one key past a chunk, a tile and a workgroup: the last chunk, tile and workgroup hold ONE row
  (577, 32)              ragged in both directions: 577 = 9 * 64 + 1 = 2 * 256 + 65 = 4 * 128 + 65
  (1024, 64)             tile-, chunk- and workgroup-exact
  (1025, 16)             one past the exact size
  (2048, 32)             the upper edge
B = 4 with mattn_ref.pad_lengths (clouds of T, T//2 + 1, 1 and 33 tokens: padded keys, a one-token cloud, dead rows; B * H * ny is a
multiple of 8, so the workgroup remap is taken), `sparse` once more at B = 3 (remap not taken), H = 6, both dtypes.

Bars: max(mattn_ref.BARS, 3 x the restatement's own distance from fp64) for EVERY case and metric -- a reduction over 2048 keys may
push the fp32 restatement itself past 1e-5 --, the distance measured on the CPU by `measure` and committed in
tests/golden/attention_long_bars.json.  No bar is ever derived from a kernel's output."""
import os

import torch

from tests import mattn_ref as R

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_long_bars.json")

H = R.H
KINDS = ("none", "blockdiag", "anti", "sparse", "radius")
SHAPES = ((513, 64), (513, 16), (577, 32), (1024, 64), (1025, 16), (2048, 32))
LARGE_KINDS = ("blockdiag", "sparse", "radius")
LARGE_SHAPES = ((513, 16), (1024, 64))
case_id = R.case_id


def cases():
    out = []
    for dt in R.DTYPES:
        for kind in KINDS:
            for T, hd in SHAPES:
                out.append(R.Case("base", kind, T, hd, 4, dt))
        out.append(R.Case("base", "sparse", 513, 16, 3, dt))
        for variant in ("amp", "adv"):
            for kind in LARGE_KINDS:
                for T, hd in LARGE_SHAPES:
                    out.append(R.Case(variant, kind, T, hd, 4, dt))
    return out


def inputs(c):
    """mattn_ref.inputs, plus the kind `none`: the tensors of the `anti` case of the same shape under an all-false mask."""
    if c.kind != "none":
        return R.inputs(c)
    qkv, dout, mask, clean = R.inputs(c._replace(kind="anti"))
    return qkv, dout, torch.zeros_like(mask), clean


def bars(c, measured):
    b = dict(R.BARS[c.dtype])
    for k in measured:
        b[k] = max(b[k], 3.0 * measured[k])
    return b


def reference(c, clean, dout, mask):
    """fp64 (out, lse, dqkv) of the case, cloud by cloud (a cloud's (H,T,T) fp64 tensors are 200 MB at T = 2048) on clean's device."""
    scale = c.hd ** -0.5
    parts = [R.reference_grad(clean[b:b + 1].double(), mask[b:b + 1], H, c.hd, scale, dout[b:b + 1].double()) for b in range(c.B)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def measure(c):
    """CPU: the restatement of the case's mode (mattn_ref.restate_f32 / emulate_bf16) against fp64 -> {metric: error}.  One thread,
    cloud by cloud: the figures are those of one fixed summation order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        qkv, dout, mask, clean = inputs(c)
        scale = c.hd ** -0.5
        ref = reference(c, clean, dout, mask)
        fn = R.emulate_bf16 if c.dtype == "bf16" else R.restate_f32
        parts = [fn(qkv[b:b + 1], mask[b:b + 1], H, c.hd, scale, dout[b:b + 1]) for b in range(c.B)]
        got = tuple(torch.cat([p[i] for p in parts]) for i in range(3))
        assert all(bool(torch.isfinite(t).all()) for t in got + ref), case_id(c)
        assert R.dead_rows_are_zero(*got, mask, H, c.hd), case_id(c)
        return R.errors(got, ref, clean.double(), dout.double(), mask, H, c.hd, c.dtype)
    finally:
        torch.set_num_threads(threads)

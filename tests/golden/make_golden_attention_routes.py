"""Writes tests/golden/attention_routes.json: which attention entry point the two block stacks' wrappers reach over a grid of
dtype x head_dim x mask x length, with the launch's meta dictionary and integer arguments.

No GPU: `_launch` and `_stream` of every module of the package that has them are replaced by a recorder (the idea of
make_golden_gemm_routes.py), and the wrappers run on real host tensors with B = 1, H = 2 -- the padded route's zero padding, its key
bitset and the (B,H,513) lse it hands from the forward to the backward included.  A row is the ordered [name, meta, integers] of one
forward and one backward.  The table was written by this file AT THE COMMIT BEFORE gm3d_amd/attention.py existed and must come out
byte-identical from every later one (tests/test_attention_routes_cpu.py): the wrappers are looked up under their names of that commit
first (fused._attention_fwd / _bwd, masked_stack._attn_fwd / _bwd) and under attention.fwd / bwd, with the caller's `head` / `pad`
(CALLERS), otherwise.

    python -m tests.golden.make_golden_attention_routes
"""
import contextlib
import json
import os
import sys

import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_routes.json")
B, H = 1, 2
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
HDS = (16, 32, 64)
TS = (1, 32, 33, 64, 65, 128, 129, 256, 257, 480, 481, 512, 513, 514, 2048)
# caller -> (head, pad): what fused.TransformerStackFn and masked_stack.MaskedStackFn state
CALLERS = {"stack": (True, True), "masked_stack": (True, False)}

_events = []


def _launch(name, meta, fn, *args):
    _events.append([name, meta, [a for a in args if type(a) is int]])


@contextlib.contextmanager
def recording():
    """the package's launches go to `_events` instead of a device"""
    mods = [m for n, m in sorted(sys.modules.items()) if n.startswith("gm3d_amd.") and m is not None]
    saved = [(m, n, vars(m)[n]) for m in mods for n in ("_launch", "_stream") if n in vars(m)]
    try:
        for m, n, _ in saved:
            setattr(m, n, _launch if n == "_launch" else (lambda: None))
        yield
    finally:
        for m, n, v in saved:
            setattr(m, n, v)


def wrappers(caller):
    """-> (fwd(qkv, bits, T, hd, out) -> (out, lse), bwd(qkv, bits, out, dout, lse, T, hd, dqkv)) of `caller`"""
    from gm3d_amd import fused, masked_stack
    s = 0.125
    if caller == "stack" and hasattr(fused, "_attention_fwd"):
        return (lambda qkv, bits, T, hd, out: fused._attention_fwd(qkv, B, T, H, s, out=out),
                lambda qkv, bits, out, dout, lse, T, hd, dqkv: fused._attention_bwd(qkv, out, dout, lse, B, T, H, s, dqkv=dqkv))
    if caller == "masked_stack" and hasattr(masked_stack, "_attn_fwd"):
        return (lambda qkv, bits, T, hd, out: masked_stack._attn_fwd(qkv, bits, B, T, H, hd, s, out),
                lambda qkv, bits, out, dout, lse, T, hd, dqkv: masked_stack._attn_bwd(qkv, out, dout, lse, bits, B, T, H, hd, s, dqkv))
    from gm3d_amd import attention
    head, pad = CALLERS[caller]
    return (lambda qkv, bits, T, hd, out: attention.fwd(qkv, bits, B, T, H, hd, s, out=out, head=head, pad=pad),
            lambda qkv, bits, out, dout, lse, T, hd, dqkv: attention.bwd(qkv, bits, out, dout, lse, B, T, H, hd, s, dqkv=dqkv,
                                                                         head=head, pad=pad))


def grid():
    """(caller, dtype name, hd, masked, T); the Point-MAE stack's wrappers know head_dim 64 and no mask only"""
    for caller in CALLERS:
        for dt in DTYPES:
            for hd in HDS:
                for masked in (False, True):
                    if caller == "stack" and (hd != 64 or masked):
                        continue
                    for T in TS:
                        yield caller, dt, hd, masked, T


def key(caller, dt, hd, masked, T):
    return "%s %s hd%d %s T%d" % (caller, dt, hd, "bits" if masked else "none", T)


def case(caller, dt, hd, masked, T):
    fwd, bwd = wrappers(caller)
    dtype = DTYPES[dt]
    qkv = torch.zeros(B * T, 3 * H * hd, dtype=dtype)
    out, dout = torch.zeros(B * T, H * hd, dtype=dtype), torch.zeros(B * T, H * hd, dtype=dtype)
    bits = torch.zeros(B, T, (T + 31) // 32, dtype=torch.int32) if masked else None
    del _events[:]
    with recording():
        out, lse = fwd(qkv, bits, T, hd, out)
        bwd(qkv, bits, out, dout, lse, T, hd, torch.zeros_like(qkv))
    return list(_events)


def generate():
    return {key(*c): case(*c) for c in grid()}


def dumps(table):
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in table.items()) + "\n}\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out, "w") as f:
        f.write(dumps(generate()))
    print(out, os.path.getsize(out))

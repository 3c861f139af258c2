"""Writes tests/golden/attention_launches.json: the ordered launches of everything that runs attention -- the two public ops, the
per-op MaskedAttention module, the Point-MAE block stack (fused.run_stack) and the hierarchical one (BlockStack on MaskedStackFn) --
at the smallest shapes that take each branch of the choice between the whole-head, LDS-resident, streaming, padded-streaming and
qkv-fused launches.

Needs the GPU: the cases run for real, under the recorder and the switches of make_golden_epilogue_launches.py ([name, integer
arguments] of every launch of the package, ["lib", shapes] of the library's 2-D products).  A training case is one forward + backward,
an inference case one forward.  No case asks for a launch the library refuses (those are pinned on the host by
tests/test_abi_limits_cpu.py and tests/test_attention_long_cpu.py).  The table was written by this file AT THE COMMIT BEFORE
gm3d_amd/attention.py existed and must come out identical from every later one (tests/test_gpu_attention_launches.py); the generator
names only what both sides have.

    python -m tests.golden.make_golden_attention_launches
"""
import json
import os
import sys

import torch

from tests.golden import make_golden_epilogue_launches as E

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_launches.json")
B, H = 2, 6

# name -> (family, arguments of the case, {module: {switch: value}})
CASES = {}
for _T, _dt in [(128, "bf16"), (129, "bf16"), (128, "f32"), (129, "f32"), (513, "bf16")]:
    CASES["ops.attention %s T%d" % (_dt, _T)] = ("op", {"T": _T, "dtype": _dt, "hd": 64, "masked_op": False, "bits": False}, {})
# no mask, head_dim 64, 64 tokens: the LDS-resident kernel where ops.attention and MaskedAttention run the whole-head one
CASES["ops.attention_masked hd64 T64 none"] = ("op", {"T": 64, "dtype": "bf16", "hd": 64, "masked_op": True, "bits": False}, {})
CASES["ops.attention_masked hd16 T129 bits"] = ("op", {"T": 129, "dtype": "bf16", "hd": 16, "masked_op": True, "bits": True}, {})
CASES["ops.attention_masked hd32 T513 bits"] = ("op", {"T": 513, "dtype": "bf16", "hd": 32, "masked_op": True, "bits": True}, {})
for _bits in (False, True):
    CASES["MaskedAttention hd64 T64 %s" % ("bits" if _bits else "none")] = ("module", {"bits": _bits}, {})
# 32: qkv product + whole-head kernel; 64: the qkv-fused launch; 65: past it; 300: LDS-resident forward, padded streaming backward;
# 500: padded both ways
for _T in (32, 64, 65, 300, 500):
    CASES["stack bf16 T%d" % _T] = ("stack", {"B": B, "T": _T, "dtype": "bf16", "train": True}, {})
CASES["stack f32 T300"] = ("stack", {"B": B, "T": 300, "dtype": "f32", "train": True}, {})
CASES["stack bf16 T64 B32 inference"] = ("stack", {"B": 32, "T": 64, "dtype": "bf16", "train": False}, {})     # two lock-step chains, no lse
CASES["stack bf16 T64 FUSE_QKV_ATTENTION=0"] = ("stack", {"B": B, "T": 64, "dtype": "bf16", "train": True},
                                                {"fused": {"FUSE_QKV_ATTENTION": False}})
CASES["masked_stack C96 T64 bits"] = ("masked_stack", {"C": 96, "T": 64, "bits": True, "train": True}, {})
CASES["masked_stack C384 T64 none"] = ("masked_stack", {"C": 384, "T": 64, "bits": False, "train": True}, {})
CASES["masked_stack C384 T129 none no_grad"] = ("masked_stack", {"C": 384, "T": 129, "bits": False, "train": False}, {})


def _bits(T):
    """a symmetric mask with an open diagonal, packed"""
    from gm3d_amd import ops
    m = torch.rand(B, T, T, generator=torch.Generator().manual_seed(T)) < 0.5
    m = (m | m.transpose(1, 2)) & ~torch.eye(T, dtype=torch.bool)
    return ops.pack_mask(m.cuda())


def _op(T, dtype, hd, masked_op, bits):
    from gm3d_amd import ops
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    qkv = E._randn(1, B, T, 3 * H * hd).to(dt)
    packed = _bits(T) if bits else None
    if masked_op:
        E._run(lambda q: ops.attention_masked(q, packed, H, hd ** -0.5), [qkv], True, False)
    else:
        E._run(lambda q: ops.attention(q, H, hd ** -0.5), [qkv], True, False)


def _module(bits):
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    attn = P.MaskedAttention(384, H).cuda().train()
    packed = _bits(64) if bits else None
    E._run(lambda x: attn(x.bfloat16(), packed), [E._randn(1, B, 64, 384)], True, True)


def _stack(B, T, dtype, train):
    E._stack(B, dtype, train, T=T, depth=1)


def _masked_stack(C, T, bits, train):
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    stack = P.BlockStack(C, 1, H, [0.0]).cuda().train(train)
    packed = _bits(T) if bits else None
    E._run(lambda x, pos: stack(x.bfloat16(), pos.bfloat16(), packed), [E._randn(1, B, T, C), E._randn(2, B, T, C, scale=0.3)], train, True)


RUNNERS = {"op": _op, "module": _module, "stack": _stack, "masked_stack": _masked_stack}


def generate():
    # every module the cases launch from, loaded before the recorder looks for `_launch`
    from gm3d_amd import heads, masked_stack, models_mae_learn_loss, optim, point_m2ae  # noqa: F401
    table = {}
    for name, (family, args, sw) in CASES.items():
        del E._events[:]
        with E.switches(sw):
            RUNNERS[family](**args)
        table[name] = list(E._events)
    return table


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out, "w") as f:
        f.write(E.dumps(generate()))
    print(out, os.path.getsize(out))

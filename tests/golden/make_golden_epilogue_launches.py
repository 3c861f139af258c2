"""Writes tests/golden/epilogue_launches.json: the ordered launches of the three autograd nodes whose dense products carry a fused
epilogue (fc1 + GELU, fc2 input gradient x GELU', conv + max-pool, conv3 + BatchNorm), at the smallest shapes that take each branch.

Needs the GPU: the cases run for real.  `_launch` of every module of the package that has one is wrapped by a recorder that notes
[name, integer arguments] and then launches; the library's 2-D products (Tensor @ Tensor, what gemm.mm ends in for fp32 operands) note
["lib", the two shapes], so that the host order of a product and the row pass behind it is on record in fp32 too.  A training case is
one forward + backward, an inference case one forward.  The table was written by this file AT THE COMMIT BEFORE the fused-epilogue
products were decided in gemm.py and must come out identical from every later one (tests/test_gpu_epilogue_launches.py);
tests/test_epilogue_routes_cpu.py asks gemm.route_* about every fused-epilogue launch in it.

The deeper Point-M2AE token embeds (96 -> 192, 192 -> 384; groups of 8) do not run on EmbedFn: their cases record the plain products
those widths reach.

    python -m tests.golden.make_golden_epilogue_launches
"""
import contextlib
import json
import os
import sys

import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "epilogue_launches.json")
_events = []

# name -> (family, arguments of the case, {module: {switch: value}})
CASES = {}
for _name, _B, _dt, _train, _sw in [
        ("B2 bf16", 2, "bf16", True, {}),                                            # R = 128: 64-row DMA tiles
        ("B65 bf16", 65, "bf16", True, {}),                                          # R = 4160: 128-row DMA tiles
        ("B2 bf16 USE_DMA=0", 2, "bf16", True, {"gemm": {"USE_DMA": False}}),        # the tiled forms
        ("B2 bf16 FUSE_GELU=0 FUSE_GELU_BWD=0", 2, "bf16", True, {"gemm": {"FUSE_GELU": False, "FUSE_GELU_BWD": False}}),
        ("B2 f32", 2, "f32", True, {}),
        ("B32 bf16 inference", 32, "bf16", False, {}),                               # two lock-step chains of 16 clouds
        ("B32 f32 inference", 32, "f32", False, {}),
        ("B32 bf16 inference FUSE_GELU=0", 32, "bf16", False, {"gemm": {"FUSE_GELU": False}})]:   # ... with two launches per fc1
    CASES["stack " + _name] = ("stack", {"B": _B, "dtype": _dt, "train": _train}, _sw)
for _C, _H, _sw in [(96, 6, {}), (128, 8, {}), (192, 6, {}), (384, 6, {}), (192, 6, {"masked_stack": {"FUSE_GELU": False}})]:
    CASES["masked C%d%s" % (_C, " FUSE_GELU=0" if _sw else "")] = ("masked", {"C": _C, "H": _H}, _sw)
for _k, _B, _G in [(32, 1, 64), (32, 16, 64), (16, 4, 512), (16, 2, 512)]:
    for _train in (True, False):
        CASES["embed k%d rows%d %s" % (_k, _B * _G * _k, "train" if _train else "eval")] = (
            "embed", {"k": _k, "B": _B, "G": _G, "train": _train, "V": None}, {})
for _train in (True, False):
    CASES["embed k32 rows32768 %s vis25" % ("train" if _train else "eval")] = (
        "embed", {"k": 32, "B": 16, "G": 64, "train": _train, "V": 25}, {})
for _B in (1, 16):
    CASES["embed k32 rows%d train FUSE_POOL=0" % (_B * 2048)] = (
        "embed", {"k": 32, "B": _B, "G": 64, "train": True, "V": None}, {"gemm": {"FUSE_POOL": False}})
CASES["embed k32 rows2048 train POOL_ON_DMA=0"] = (
    "embed", {"k": 32, "B": 1, "G": 64, "train": True, "V": None}, {"gemm": {"POOL_ON_DMA": False}})
for _cin, _cout, _G in [(96, 192, 256), (192, 384, 64)]:
    CASES["embed m2ae %d->%d" % (_cin, _cout)] = ("embed_deep", {"cin": _cin, "cout": _cout, "B": 2, "G": _G, "k": 8}, {})


@contextlib.contextmanager
def switches(sw):
    import importlib
    saved = []
    try:
        for mod, kv in sw.items():
            m = importlib.import_module("gm3d_amd." + mod)
            for k, v in kv.items():
                saved.append((m, k, getattr(m, k)))
                setattr(m, k, v)
        yield
    finally:
        for m, k, v in reversed(saved):
            setattr(m, k, v)


@contextlib.contextmanager
def recording():
    """the package's launches and the library's 2-D products note themselves in `_events`, then run"""
    mods = [m for n, m in sorted(sys.modules.items()) if n.startswith("gm3d_amd.") and m is not None and "_launch" in vars(m)]
    saved = [(m, m._launch) for m in mods]
    own = "__matmul__" in vars(torch.Tensor)
    matmul = torch.Tensor.__matmul__

    def wrap(orig):
        def _launch(name, meta, fn, *args):
            _events.append([name, [a for a in args if type(a) is int]])
            return orig(name, meta, fn, *args)
        return _launch

    def noted_matmul(a, b):
        _events.append(["lib", list(a.shape) + list(b.shape)])
        return matmul(a, b)
    try:
        for m, orig in saved:
            m._launch = wrap(orig)
        torch.Tensor.__matmul__ = noted_matmul
        yield
    finally:
        for m, orig in saved:
            m._launch = orig
        if own:
            torch.Tensor.__matmul__ = matmul
        else:
            del torch.Tensor.__matmul__


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _run(fn, inputs, train, bf16):
    """one forward (+ backward of the sum) of fn(*inputs) with the launches on record"""
    inputs = [t.requires_grad_(train) if t.is_floating_point() else t for t in inputs]
    with recording():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16), torch.set_grad_enabled(train):
            out = fn(*inputs)
        if train:
            out.float().sum().backward()
        torch.cuda.synchronize()


def _stack(B, dtype, train, T=64, depth=2):
    from gm3d_amd import fused
    from gm3d_amd import models_mae_learn_loss as M
    torch.manual_seed(0)
    dec = M.TransformerDecoder(embed_dim=384, depth=depth, drop_path_rate=0.0, num_heads=6).cuda().train(train)
    # bf16 shadows of the blocks' weights at a constant stride in ONE buffer, like the flat optimizer's: whether the backward's
    # transposing launch takes them must not depend on where the allocator happens to put separately cast copies
    ws = [[p for p in fused.block_params(b) if p.dim() == 2] for b in dec.blocks]
    per = sum(p.numel() for p in ws[0])
    flat = torch.empty(len(ws) * per, dtype=torch.bfloat16, device="cuda")
    for i, row in enumerate(ws):
        off = i * per
        for p in row:
            shadow = flat[off:off + p.numel()].view_as(p).copy_(p.detach())
            fused.weight_cache.pin_view(p, shadow)
            off += p.numel()
    _run(lambda x, pos: fused.run_stack(dec.blocks, dec.norm, x, pos, train), [_randn(1, B, T, 384), _randn(2, B, T, 384)], train,
         dtype == "bf16")


def _masked(C, H):
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    stack = P.BlockStack(C, 1, H, [0.0]).cuda().train()
    _run(lambda x, pos: stack(x.bfloat16(), pos.bfloat16(), None), [_randn(1, 2, 64, C), _randn(2, 2, 64, C, scale=0.3)], True, True)


def _embed(k, B, G, train, V):
    from gm3d_amd import embed
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    enc = (M.Encoder(384) if k == 32 else P.TokenEmbed(3, 96)).cuda().train(train)
    vis = None
    if V:
        vis = torch.stack([torch.randperm(G, generator=torch.Generator().manual_seed(b))[:V] for b in range(B)]).cuda()
    _run(lambda nb: embed.run_embed(enc, nb, vis_ids=vis), [_randn(3, B, G, k, 3, scale=0.2)], train, True)


def _embed_deep(cin, cout, B, G, k):
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    enc = P.TokenEmbed(cin, cout).cuda().train()
    _run(enc, [_randn(4, B, G, k, cin, scale=0.5)], True, True)


RUNNERS = {"stack": _stack, "masked": _masked, "embed": _embed, "embed_deep": _embed_deep}


def generate():
    # every module the cases launch from, loaded before the recorder looks for `_launch`
    from gm3d_amd import heads, masked_stack, models_mae_learn_loss, optim, point_m2ae  # noqa: F401
    table = {}
    for name, (family, args, sw) in CASES.items():
        del _events[:]
        with switches(sw):
            RUNNERS[family](**args)
        table[name] = list(_events)
    return table


def dumps(table):
    return "{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(out, "w") as f:
        f.write(dumps(generate()))
    print(out, os.path.getsize(out))

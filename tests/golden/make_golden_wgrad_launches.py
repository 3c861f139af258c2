"""Writes tests/golden/wgrad_launches.json: the ordered weight-gradient launches (dW = dy^T @ x) of the training steps and of the
mini-PointNet embed, with the fork and the join of the backward region's side stream, at the smallest shapes that take each branch
of the scheduling: forked, deferred, in line, per-request fallback, the embed's node-local batch of four, one and none.

Needs the GPU: the cases run for real.  `_launch` of every module of the package that has one is wrapped by a recorder (the idea of
make_golden_epilogue_launches.py) that keeps the launches of the weight-gradient family

    gm3d_gemm_nt_*  gm3d_sum_few_rows  gm3d_pad_cols      [name, integer arguments, "main" | "side"]
    gm3d_gemm_nt_bf16_multi                               ... and {"problems": [(nb, R, N, K), ...], "splits": [...]} behind them

("side": the current stream is not the one the case started on), torch.bmm -- in the package only the library form of a weight
gradient calls it -- as ["lib bmm", the two shapes, stream], and streams.fork / streams.join of the region's stream as ["fork"] /
["join"].  The other launches of a step are pinned by epilogue_launches.json and are left out here.

The table was written by this file AT THE COMMIT BEFORE gm3d_amd/wgrads.py existed and must come out identical from every later one
(tests/test_gpu_wgrad_launches.py); tests/test_wgrad_routes_cpu.py asks gemm.multi_splits about every combined launch in it.  The
generator therefore names only what both sides have (model constructors, the engines' step functions, embed.run_embed), and a
switch is set wherever it lives (`HOMES`, the newer home first).

    python -m tests.golden.make_golden_wgrad_launches
"""
import contextlib
import importlib
import json
import os
import sys
from types import SimpleNamespace

import torch

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrad_launches.json")
HOMES = ("wgrads", "fused", "gemm", "point_m2ae")
KEPT = ("gm3d_sum_few_rows", "gm3d_pad_cols")
_events = []

# name -> (family, arguments of the case, {switch: value})
CASES = {
    # encoder rows 25 x 32 = 800: the encoder forks, the 4-block decoders are deferred to it -> one combined launch
    "northstar B32": ("northstar", {"B": 32}, {}),
    # encoder rows 200, no multiple of 32: the combined list falls back per request (library for the encoder, NT for the decoders)
    "northstar B8": ("northstar", {"B": 8}, {}),
    "northstar B32 ASYNC_WGRAD=0": ("northstar", {"B": 32}, {"ASYNC_WGRAD": False}),
    "northstar B32 torch AdamW": ("northstar", {"B": 32, "flat": False}, {}),                 # no slots: nothing is deferred
    "northstar B32 onto .grad": ("northstar", {"B": 32, "again": True}, {}),                # not fresh: in line, no slots
    "northstar B32 DEFER_HEAD_WGRAD=1": ("northstar", {"B": 32}, {"DEFER_HEAD_WGRAD": True}),
    "northstar B32 MULTI_WGRAD=0": ("northstar", {"B": 32}, {"MULTI_WGRAD": False}),
    # 15 layer requests deferred to ONE launch at the exit (four more layers do not qualify and run in line); the masked stacks take
    # no part in the region.  No step defers more than 16: the chunks are asked directly in tests/test_gpu_wgrad_launches.py
    "m2ae B2": ("m2ae", {"B": 2}, {}),
    "m2ae B2 DEFER_WGRADS=0": ("m2ae", {"B": 2}, {"DEFER_WGRADS": False}),
    "embed k32 rows2048 bf16": ("embed", {"k": 32, "B": 1, "G": 64, "bf16": True}, {}),     # four requests, one launch
    "embed k32 rows2048 f32": ("embed", {"k": 32, "B": 1, "G": 64, "bf16": False}, {}),     # none batched
    "embed k32 rows2048 bf16 MULTI_WGRAD=0": ("embed", {"k": 32, "B": 1, "G": 64, "bf16": True}, {"MULTI_WGRAD": False}),
    "embed k16 rows16384 bf16": ("embed", {"k": 16, "B": 2, "G": 512, "bf16": True}, {}),   # the Point-M2AE token embed
    # 80 rows, 5 groups, 2 of them visible: only conv4's 32 rows are a multiple of 32 -> ONE request, alone on its own splits
    "embed k16 rows80 vis2 bf16": ("embed", {"k": 16, "B": 1, "G": 5, "bf16": True, "V": 2}, {}),
}


def home(switch):
    """the module of the package that holds `switch`: the first of HOMES that exists and has it"""
    for name in HOMES:
        try:
            m = importlib.import_module("gm3d_amd." + name)
        except ImportError:
            continue
        if hasattr(m, switch):
            return m
    raise AttributeError(switch)


@contextlib.contextmanager
def switches(sw):
    saved = []
    try:
        for k, v in sw.items():
            m = home(k)
            saved.append((m, k, getattr(m, k)))
            setattr(m, k, v)
        yield
    finally:
        for m, k, v in reversed(saved):
            setattr(m, k, v)


@contextlib.contextmanager
def recording():
    """the weight-gradient launches, the library's batched products and the region stream's fork / join note themselves, then run"""
    from gm3d_amd import streams
    mods = [m for n, m in sorted(sys.modules.items()) if n.startswith("gm3d_amd.") and m is not None and "_launch" in vars(m)]
    saved = [(m, "_launch", m._launch) for m in mods] + [(torch, "bmm", torch.bmm), (streams, "fork", streams.fork),
                                                          (streams, "join", streams.join)]
    start = torch.cuda.current_stream().cuda_stream
    forked = set()

    def where():
        return "main" if torch.cuda.current_stream().cuda_stream == start else "side"

    def wrap(orig):
        def _launch(name, meta, fn, *args):
            if name.startswith("gm3d_gemm_nt_") or name in KEPT:
                ev = [name, [a for a in args if type(a) is int], where()]
                if "problems" in meta:
                    ev.append({"problems": [list(p) for p in meta["problems"]], "splits": list(meta["splits"])})
                _events.append(ev)
            return orig(name, meta, fn, *args)
        return _launch

    def bmm(a, b, **kw):
        _events.append(["lib bmm", list(a.shape) + list(b.shape), where()])
        return saved[-3][2](a, b, **kw)

    def fork(side, origin=None, who=None):
        if who and "weight-gradient stream" in who:
            forked.add(side.cuda_stream)
            _events.append(["fork", [], where()])
        return saved[-2][2](side, origin, who)

    def join(side, into=None):
        if side.cuda_stream in forked:
            _events.append(["join", [], where()])
        return saved[-1][2](side, into)
    try:
        for m, n, orig in saved[:-3]:
            setattr(m, n, wrap(orig))
        torch.bmm, streams.fork, streams.join = bmm, fork, join
        yield
    finally:
        for m, n, orig in saved:
            setattr(m, n, orig)


def _randn(seed, *shape, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _no_drop_path(model):
    for m in model.modules():
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0
    return model


def _northstar(B, flat=True, again=False):
    """one step after one warm-up step.  again: the recorded backward is a further one onto the gradients of the step before it (the
    engine asked not to zero them: no optimizer, not the first micro-batch), with the flat optimizer's slots still registered"""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=40)
    torch.manual_seed(0)
    model = _no_drop_path(M.mae_vit_base_patch16_dec512d8b().cuda().train())
    ema = E.ModelEma(model, 0.999)
    opt = E.build_optimizer(model, lr=1e-3, flat=flat, model_ema=ema if flat else None)
    x = _randn(1, B, 1024, 3, scale=0.3)
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(2)).cuda()

    def step(**kw):
        kw.setdefault("optimizer", opt)
        return E.step_forward_backward(model, ema, x.clone(), 200, args, augment=False, mask_noise=noise, **kw)
    step()
    E.step_update(model, ema, opt)
    if again:
        step()
    with recording():
        step(**({"optimizer": None, "accum_first": False} if again else {}))
        torch.cuda.synchronize()


def _m2ae(B):
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import point_m2ae as P
    args = SimpleNamespace(bf16=True, epochs=300, lr=1e-3, min_lr=1e-6, warmup_epochs=10, accum_iter=1, seed=0)
    torch.manual_seed(0)
    model = _no_drop_path(P.PointM2AE().cuda().train())
    opt, ema = EM.build_optimizer(model, lr=1e-3)
    pts = _randn(5, B, 2048, 3, scale=0.3)
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(6)).cuda()
    P.pretrain_step(model, ema, opt, pts.clone(), 100, args, mask_noise=noise, augment=False)
    with recording():
        P.pretrain_step(model, ema, opt, pts.clone(), 100, args, mask_noise=noise, augment=False)
        torch.cuda.synchronize()


def _embed(k, B, G, bf16, V=None):
    from gm3d_amd import embed
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    enc = (M.Encoder(384) if k == 32 else P.TokenEmbed(3, 96)).cuda().train()
    nb = _randn(3, B, G, k, 3, scale=0.2).requires_grad_(True)
    vis = torch.stack([torch.randperm(G, generator=torch.Generator().manual_seed(b))[:V] for b in range(B)]).cuda() if V else None
    with recording():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            out = embed.run_embed(enc, nb, vis_ids=vis)
        out.float().sum().backward()
        torch.cuda.synchronize()


RUNNERS = {"northstar": _northstar, "m2ae": _m2ae, "embed": _embed}


def generate(only=None):
    # every module the cases launch from, loaded before the recorder looks for `_launch`
    from gm3d_amd import engine_pretrain_m2ae, heads, masked_stack, models_mae_learn_loss, optim, point_m2ae  # noqa: F401
    table = {}
    for name, (family, args, sw) in CASES.items():
        if only is not None and name not in only:
            continue
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

"""What the soft-target kernels cost (gm3d_amd/losses.py, csrc/soft_ce.hip): five runs of each measurement, median and min-max.

  (a) loss forward + backward, one launch each, at (B,C) = (32,40) and (64,15), against the aten chain that restates timm's
      LabelSmoothingCrossEntropy (log_softmax, gather, mean, two scaled adds, mean, and autograd's backward of them);
  (b) the mixing launch at B = 32, N = 1024 against index_select + two scaled products + add;
  (c) the replayed PointTransformer fine-tune step at tools/bench_finetune.py's shape (flat optimizer, bf16) with smoothing + mixup
      against the plain cross-entropy step, the two alternating in this process; --parent-ms takes the graph_flat_ms figures
      tools/bench_finetune.py printed on the parent commit, and the comparison is stated against their spread.

(a) and (b) are timed twice: as a hipGraph of REP repetitions replayed between two events (device time per repetition: what a captured
step pays) and eagerly with a host clock around a synchronised loop (what an un-captured step pays, launch overhead included).
python tools/bench_soft_targets.py [--batch 32] [--steps 20] [--parent-ms 4.15,4.17,...] [--out profiles/soft_targets_bench.json]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from types import SimpleNamespace
from gm3d_amd import engine_finetune as EF, losses as L, streams
from gm3d_amd.point_transformer import PointTransformer
from bench import make_clouds

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--points", type=int, default=8192)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--parent-ms", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: nothing here is a CPU measurement"
dev = torch.device("cuda")
REP, EAGER_ITERS = 200, 2000


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": [round(x, 4) for x in xs]}


def graph_us(fn):
    """device microseconds per call of fn inside a replayed graph of REP calls"""
    streams.warm_up(fn, 3)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with streams.capture(g):
        for _ in range(REP):
            fn()
    out = []
    for _ in range(a.runs + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(5):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / (5 * REP))
    return spread(out[1:])


def eager_us(fn):
    for _ in range(50):
        fn()
    out = []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(EAGER_ITERS):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / EAGER_ITERS)
    return spread(out)


res = {"metric": "soft targets: loss fwd+bwd (us), mixing launch (us), replayed fine-tune step (ms)", "runs": a.runs}

# ---- (a) the loss node against the aten chain
S = 0.1
for B, C in ((32, 40), (64, 15)):
    z = torch.randn(B, C, device=dev, requires_grad=True)
    y = torch.randint(0, C, (B,), device=dev)
    crit = L.LabelSmoothingCrossEntropy(S)
    crit(z.detach(), y)                                        # stages the coefficients once, outside any capture

    def ours():
        return torch.autograd.grad(crit(z, y), z)[0]

    def aten():                                                 # timm.loss.LabelSmoothingCrossEntropy.forward
        logp = F.log_softmax(z, dim=-1)
        nll = -logp.gather(dim=-1, index=y.unsqueeze(1)).squeeze(1)
        loss = ((1.0 - S) * nll + S * (-logp.mean(dim=-1))).mean()
        return torch.autograd.grad(loss, z)[0]

    assert float((ours() - aten()).abs().max()) <= 1e-6
    res["loss_fwd_bwd_B%d_C%d" % (B, C)] = {"kernels_graph_us": graph_us(ours), "aten_graph_us": graph_us(aten),
                                           "kernels_eager_us": eager_us(ours), "aten_eager_us": eager_us(aten)}

# ---- (b) the mixing launch against index_select + two scaled products + add
x = torch.randn(32, 1024, 3, device=dev)
lab = torch.randint(0, 40, (32,), device=dev)
mix = L.PointMixup(0.2, rng=np.random.RandomState(0), generator=torch.Generator().manual_seed(0))
lam, perm = mix.draw(32, dev)
dperm = perm.to(dev)
ours_mix = lambda: mix.mix(x, lab)[0]
aten_mix = lambda: lam * x + (1 - lam) * x.index_select(0, dperm)      # lam is a host value here: a capture would freeze it
assert torch.equal(ours_mix(), aten_mix())
res["mixup_B32_N1024"] = {"kernel_graph_us": graph_us(ours_mix), "aten_graph_us": graph_us(aten_mix),
                          "kernel_eager_us": eager_us(ours_mix), "aten_eager_us": eager_us(aten_mix)}

# ---- (c) the replayed fine-tune step, plain cross-entropy against smoothing + mixup, alternating
torch.manual_seed(0)
cfg = dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64, encoder_dims=384)
args = SimpleNamespace(lr=5e-4, min_lr=1e-6, warmup_epochs=10, epochs=300)
pool = [make_clouds(a.batch, a.points, 100 + i, dev) for i in range(3)]
targets = (torch.arange(a.batch, device=dev) * 7) % 40


def make_step(crit, mixup):
    model = PointTransformer(cfg).to(dev).train()
    opt = EF.build_optimizer(model, lr=5e-4, flat=True, max_norm=10.0)
    g = EF.GraphedFinetuneStep(model, crit, opt, pool[0], targets, npoints=1024, max_norm=10.0, bf16=True, mixup=mixup)

    def step(i):
        EF.adjust_learning_rate(opt, 20 + i / 100.0, args)
        return g(pool[i % 3], targets)
    return step


def timed_ms(step):
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        out = step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"]))
    return dt / a.steps * 1e3


plain = make_step(nn.CrossEntropyLoss(), None)
soft = make_step(L.LabelSmoothingCrossEntropy(S), L.PointMixup(0.2, rng=np.random.RandomState(1), generator=torch.Generator().manual_seed(1)))
pm, sm = [], []
for _ in range(a.runs):
    pm.append(timed_ms(plain))
    sm.append(timed_ms(soft))
step = {"batch": a.batch, "steps": a.steps, "plain_ce_graph_flat_ms": spread(pm), "smoothing_mixup_graph_flat_ms": spread(sm)}
if a.parent_ms:
    step["parent_commit_graph_flat_ms"] = spread([float(v) for v in a.parent_ms.split(",")])
step["extra_ms_median"] = round(step["smoothing_mixup_graph_flat_ms"]["median"] - step["plain_ce_graph_flat_ms"]["median"], 4)
res["finetune_step"] = step
line = json.dumps(res)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
print(line)

"""Voting evaluation throughput (P/tools/runner_finetune.py:271-335) at the ModelNet40 test shape: B clouds of 8192 points,
npoints 1024, V votes, 40 classes, bf16.  Three forms over the same batches:
  (a) reference  -- the reference's loop: V eager forwards of B clouds through model(points), torch index_select / gather /
                    per-cloud scale-and-translate, torch mean + argmax;
  (b) batched    -- engine_finetune.vote_batch, eager: vote_sample, ONE forward over V*B clouds, cls_tail_vote;
  (c) graphed    -- GraphedVoteEval: (b) captured once, one replay per batch.
Clouds/s is over a host clock around whole batches ending in a device synchronise (host draws included); launches per batch are
the HIP runtime launch calls (kernel launches + graph launches) the profiler sees for one batch.
python tools/bench_vote.py [--batch 32] [--votes 10] [--iters 10]     (GPU box; prints one JSON line)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gm3d_amd import engine_finetune as EF, ops
from gm3d_amd.point_transformer import PointTransformer
from bench import make_clouds

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--votes", type=int, default=10)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--points", type=int, default=8192)
a = ap.parse_args()
dev = torch.device("cuda")
torch.manual_seed(0)
cfg = dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64, encoder_dims=384)
model = PointTransformer(cfg).to(dev).eval()
B, V, NP = a.batch, a.votes, 1024
P = EF.vote_point_all(NP, a.points)
pool = [make_clouds(B, a.points, 300 + i, dev) for i in range(3)]
labels = (torch.arange(B, device=dev) * 7) % 40
rng = np.random.RandomState(0)


@torch.no_grad()
def reference(points):
    fps_idx = ops.furthest_point_sample(points, P)
    votes = []
    for _ in range(V):
        idx = fps_idx[:, torch.from_numpy(rng.choice(P, NP, False)).to(dev)].contiguous()
        pts = ops.gather_operation(points.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        for i in range(B):
            xyz1, xyz2 = rng.uniform(2. / 3., 3. / 2., [3]), rng.uniform(-0.2, 0.2, [3])
            pts[i, :, 0:3] = torch.mul(pts[i, :, 0:3], torch.from_numpy(xyz1).float().to(dev)) + torch.from_numpy(xyz2).float().to(dev)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            votes.append(model(pts).float().unsqueeze(0))
    return torch.cat(votes).mean(0).argmax(-1)


draws = EF._VoteDraws(V, NP, B, dev)
counter = torch.zeros(1, dtype=torch.long, device=dev)


@torch.no_grad()
def batched(points):
    draws.stage(rng, P)
    return EF.vote_batch(model, points, labels, draws.subsets, draws.scale, draws.shift, P, counter, bf16=True)[1]


graphed_eval = EF.GraphedVoteEval(model, pool[0], labels, npoints=NP, times=V, bf16=True, rng=rng)


def graphed(points):
    return graphed_eval(points, labels)[1]


def launches(fn):
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn(pool[0])
        torch.cuda.synchronize()
    n_launch = n_graph = n_kernels = 0
    for ev in prof.events():
        name = ev.name
        if "GraphLaunch" in name:
            n_graph += 1
        elif "LaunchKernel" in name:
            n_launch += 1
        elif getattr(ev, "device_type", None) == torch.autograd.DeviceType.CUDA:
            n_kernels += 1
    return {"kernel_launch_calls": n_launch, "graph_launch_calls": n_graph, "device_activities": n_kernels}


res = {"box": torch.cuda.get_device_name(0), "batch": B, "votes": V, "points": a.points, "npoints": NP, "bf16": True}
forms = {"reference": reference, "batched": batched, "graphed": graphed}
for name, fn in forms.items():
    for i in range(a.warmup):
        fn(pool[i % 3])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.iters):
        fn(pool[i % 3])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res[name] = {"clouds_per_s": round(B * a.iters / dt, 1), "ms_per_batch": round(1e3 * dt / a.iters, 3)}
for name, fn in forms.items():
    res[name].update(launches(fn))
print(json.dumps(res))

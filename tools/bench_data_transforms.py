"""Augmentation chain A (Scale -> Translate -> Jitter -> RandomInputDropout -> RandomHorizontalFlip) on one batch of 128 x 1024
points: gm3d_amd.data_transforms.Compose (three draw calls and one gm3d_augment launch) beside the reference's per-cloud loops.

 (a) fused: wall time per call over --calls back-to-back calls ending in one synchronise (draws + launch, as an engine issues
     them), the GPU time of one call (draws + launch) and of the launch alone from HIP events, and the same call replayed from a
     captured graph;
 (b) the reference's transforms restated for the same GPU tensor (datasets/data_transforms.py: per cloud np.random / random draws
     on the host, a host-to-device copy of every draw, `.tolist()` indexing in the dropout, torch.max in the flip): wall time per
     call over --ref-calls calls ending in one synchronise.
Method of tools/bench_knn_probe.py: one warm-up, --repeats runs, median and min-max.  Writes profiles/data_transforms_bench.json and
prints it as one JSON line.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def wall(fn, calls, repeats):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls
    run()
    return spread([run() for _ in range(repeats)])


def events(fn, calls, repeats):
    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 1e3 / calls
    run()
    return spread([run() for _ in range(repeats)])


def reference_chain_a(pc, lo=2. / 3., hi=3. / 2., t=0.2, std=0.01, clip=0.05, max_ratio=0.5):
    """What the reference's five transforms do to a (B,N,3) GPU tensor, one transform after the other, each cloud by cloud."""
    B, N = pc.shape[0], pc.shape[1]
    for i in range(B):                                         # PointcloudScale: three host draws, copied over, per cloud
        scale = torch.from_numpy(np.random.uniform(low=lo, high=hi, size=[3])).float().cuda()
        pc[i] = pc[i] * scale
    for i in range(B):                                         # PointcloudTranslate
        shift = torch.from_numpy(np.random.uniform(low=-t, high=t, size=[3])).float().cuda()
        pc[i] = pc[i] + shift
    for i in range(B):                                         # PointcloudJitter: one normal_ fill and one clamp per cloud
        pc[i] += pc.new(N, 3).normal_(mean=0.0, std=std).clamp_(-clip, clip)
    for i in range(B):                                         # PointcloudRandomInputDropout: host draws, a Python index list
        ratio = np.random.random() * max_ratio
        dropped = np.where(np.random.random((N,)) <= ratio)[0]
        if len(dropped) > 0:
            pc[i][dropped.tolist()] = pc[i][0].repeat(len(dropped), 1)
    for i in range(B):                                         # RandomHorizontalFlip (upright z): a torch.max per flipped axis
        if random.random() < 0.95:
            for ax in (0, 1):
                if random.random() < 0.5:
                    pc[i, :, ax] = torch.max(pc[i, :, ax]) - pc[i, :, ax]
    return pc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--ref-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_transforms_bench.json"))
    args = ap.parse_args()
    from gm3d_amd import data_transforms as T
    from gm3d_amd._capi import check, lib
    from gm3d_amd.ops import _ptr, _stream
    B, N = args.batch, args.points
    chain = T.Compose([T.PointcloudScale(), T.PointcloudTranslate(), T.PointcloudJitter(), T.PointcloudRandomInputDropout(),
                       T.RandomHorizontalFlip()])
    gen = torch.Generator(device="cuda").manual_seed(0)
    src = torch.randn(B, N, 3, device="cuda", generator=gen) * 0.3
    pc = src.clone()
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "points": N, "chain": [type(t).__name__ for t in chain.transforms],
           "calls_per_run": args.calls, "ref_calls_per_run": args.ref_calls}

    # ---- (a) the fused launch
    res["a_fused_s"] = {"wall_per_call": wall(lambda: chain(pc, generator=gen), args.calls, args.repeats),
                        "gpu_per_call": events(lambda: chain(pc, generator=gen), args.calls, args.repeats)}
    prog = T.Program(chain.transforms)
    cloud_u, point_u, point_z = chain.draw(prog, B, N, pc.device, [None] * len(prog), gen)
    ops = (ctypes.c_int * len(prog))(*prog.codes)
    params = (ctypes.c_float * (3 * len(prog)))(*[v for p in prog.params for v in p])
    pc.copy_(src)

    def launch():
        check(lib.gm3d_augment(_ptr(pc), B, N, len(prog), ops, params, _ptr(cloud_u), _ptr(point_u), _ptr(point_z), _stream()), "gm3d_augment")
    res["a_fused_s"]["gpu_launch_alone"] = events(launch, args.calls, args.repeats)
    pc.copy_(src)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(gen)
    with torch.cuda.graph(graph):
        chain(pc, generator=gen)
    res["a_fused_s"]["wall_per_replay"] = wall(graph.replay, args.calls, args.repeats)
    del graph

    # ---- (b) the reference's loops on the same tensor
    np.random.seed(0)
    random.seed(0)
    pc.copy_(src)
    res["b_reference_loops_s"] = {"wall_per_call": wall(lambda: reference_chain_a(pc), args.ref_calls, args.repeats)}
    res["reference_over_fused_wall"] = (res["b_reference_loops_s"]["wall_per_call"]["median"]
                                        / res["a_fused_s"]["wall_per_call"]["median"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

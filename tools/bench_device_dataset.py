"""Device-resident dataset (gm3d_amd/data.py, gm3d_sample_normalize) beside the reference's host data path, and under the engine.

Synthetic ShapeNet55-shaped clouds (8192 points each, fixed seed), batches of 128 clouds sampled down to 1024 points and normalised:
 (a) one DeviceLoader batch: wall time per batch over an epoch of the loader (torch.rand + one launch per batch, one synchronise
     at the end), and the GPU time of the key draw and of the launch from HIP events;
 (b) the reference's host path restated for the same arrays held in host memory (per sample: an in-place shuffle of an 8192-long
     permutation, a fancy-index gather, pc_norm; datasets/ShapeNet55Dataset.py:45-67), collated by a torch DataLoader with the
     reference's 8 workers and copied to the device: wall time per batch over an epoch, with and without the workers' start-up;
 (c) engine_pretrain_point_mae.train_one_epoch over a DeviceLoader against the same engine over a list of ready-made device
     batches, alternating, after the engine has captured its step.
Method of tools/bench_knn_probe.py: one warm-up, --repeats runs, median and min-max.  Writes profiles/device_dataset_bench.json and
prints it as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def synthetic(M, N0, seed=0):
    """M gaussian clouds, each scaled and shifted on its own (the normalisation has work to do)."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((M, N0, 3)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (M, 1, 1)).astype(np.float32)
    x += rng.uniform(-1.0, 1.0, (M, 1, 3)).astype(np.float32)
    return x


class HostShapeNet(torch.utils.data.Dataset):
    """The reference's ShapeNet.__getitem__ on clouds already in host memory (its np.load is left out: in favour of the host path)."""

    def __init__(self, clouds, num):
        self.clouds, self.num = clouds, num
        self.permutation = np.arange(clouds.shape[1])

    def __len__(self):
        return len(self.clouds)

    def __getitem__(self, i):
        np.random.shuffle(self.permutation)
        pc = self.clouds[i][self.permutation[:self.num]]
        pc = pc - np.mean(pc, axis=0)
        pc = pc / np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
        return torch.from_numpy(pc).float()


def device_epoch(loader, epoch):
    loader.set_epoch(epoch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for batch in loader:
        last = batch
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / len(loader), last


def host_epoch(loader):
    """-> (seconds per batch over the whole epoch, seconds per batch after the first one arrived)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t1, n = None, 0
    for batch in loader:
        batch = batch.cuda(non_blocking=True)
        n += 1
        if t1 is None:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / n, (t2 - t1) / max(n - 1, 1)


def events(fn, repeats):
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return spread(ts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--clouds", type=int, default=2048, help="clouds in the dataset of (a) and (b)")
    ap.add_argument("--engine-clouds", type=int, default=8192, help="clouds in the dataset of (c)")
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_dataset_bench.json"))
    args = ap.parse_args()
    from gm3d_amd import data as D
    B, N0, num = args.batch, args.points, args.npoints
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "points": N0, "npoints": num, "normalize": True,
           "clouds": args.clouds, "cpus": len(os.sched_getaffinity(0)), "workers": args.workers}

    # ---- (a) one DeviceLoader batch
    host = synthetic(args.clouds, N0)
    ds = D.DeviceDataset.from_arrays(host, npoints=num, normalize=True)
    loader = D.DeviceLoader(ds, B, seed=0)
    device_epoch(loader, 0)                                    # warm-up: module load, LDS attribute, allocator
    runs = [device_epoch(loader, e + 1)[0] for e in range(args.repeats)]
    idx = torch.arange(B, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    keys = torch.rand((B, N0), generator=gen, device="cuda")
    res["a_device_batch_s"] = {"wall_per_batch": spread(runs), "batches_per_epoch": len(loader),
                               "gpu_rand": events(lambda: torch.rand((B, N0), generator=gen, device="cuda"), args.repeats),
                               "gpu_launch": events(lambda: D.sample_normalize(ds.points, idx, keys, num, True), args.repeats),
                               "gpu_launch_no_normalize": events(lambda: D.sample_normalize(ds.points, idx, keys, num, False),
                                                                 args.repeats)}

    # ---- (b) the reference's host path on the same arrays
    hl = torch.utils.data.DataLoader(HostShapeNet(host, num), batch_size=B, shuffle=True, drop_last=True, num_workers=args.workers)
    host_epoch(hl)
    whole, steady = zip(*[host_epoch(hl) for _ in range(args.repeats)])
    res["b_host_batch_s"] = {"wall_per_batch_whole_epoch": spread(whole), "wall_per_batch_after_first": spread(steady),
                             "batches_per_epoch": len(hl)}
    a_med = res["a_device_batch_s"]["wall_per_batch"]["median"]
    res["host_over_device"] = {"whole_epoch": statistics.median(whole) / a_med, "after_first": statistics.median(steady) / a_med}
    del hl, loader, ds

    # ---- (c) the engine over a DeviceLoader against ready-made batches
    if not args.skip_engine:
        from gm3d_amd import engine_pretrain_point_mae as EP
        from gm3d_amd.point_mae import Point_MAE
        cfg = {"group_size": 32, "num_group": 64, "loss": "cdl2",
               "transformer_config": {"mask_ratio": 0.6, "mask_type": "rand", "trans_dim": 384, "encoder_dims": 384, "depth": 12,
                                      "drop_path_rate": 0.1, "num_heads": 6, "decoder_depth": 4, "decoder_num_heads": 6}}
        torch.manual_seed(0)
        model = Point_MAE(cfg).cuda().train()
        opt = EP.build_optimizer(model)
        targs = SimpleNamespace(bf16=True, lr=1e-3, epochs=300, warmup_epochs=10, step_per_update=1)
        big = synthetic(args.engine_clouds, N0, seed=1) if args.engine_clouds != args.clouds else host
        ds = D.DeviceDataset.from_arrays(big, npoints=num, normalize=True)
        loader = D.DeviceLoader(ds, B, seed=0)
        loader.set_epoch(0)
        ready = [b.clone() for b in loader]

        def epoch(feed, e):
            if feed is loader:
                loader.set_epoch(e)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = EP.train_one_epoch(model, feed, opt, "cuda", e, targs, print_freq=10 ** 9)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / len(feed), st

        epoch(ready, 0)                                        # eager iterations, the capture
        epoch(loader, 0)
        tl, tr, replayed = [], [], True
        for e in range(args.repeats):                          # alternating
            s, st = epoch(loader, e + 1)
            tl.append(s)
            replayed = replayed and st["replayed_iters"] == len(loader)
            s, st = epoch(ready, e + 1)
            tr.append(s)
            replayed = replayed and st["replayed_iters"] == len(ready)
        res["c_engine_step_s"] = {"device_loader": spread(tl), "ready_batches": spread(tr), "iterations_per_epoch": len(loader),
                                  "clouds": args.engine_clouds, "every_iteration_replayed": replayed,
                                  "loader_over_ready": statistics.median(tl) / statistics.median(tr),
                                  "loader_clouds_per_s": B / statistics.median(tl), "ready_clouds_per_s": B / statistics.median(tr)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

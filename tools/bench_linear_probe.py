"""Linear probe: gm3d_amd.linear_probe.LinearProbe (one launch per training iteration) beside the aten chain that restates the
reference on the same GPU (torch.nn.BatchNorm1d(affine=False, eps=1e-6) + Linear + torch.optim.SGD + cross_entropy on the cached
features, fp32, the same orders, rates and initial weights; main_linprob.py:219-263).

Synthetic ModelNet40-shaped features (9,843 train / 2,468 test rows, 40 classes, 384-wide, fixed seed, offset +3), the defaults of
LinearProbe: batch 512, 90 epochs, 10 warm-up epochs, blr 0.1, evaluation after every epoch.  Wall time of a whole fit, --repeats
runs of each path (median, min, max; one warm-up fit before), the final top-1 / top-5 of both, the largest difference of the loss
trajectories.  Writes profiles/linear_probe_bench.json and prints it as one JSON line.

GPU time per launch and launches per iteration come from a run of their own: one path, a few epochs, under the profiler,
    rocprofv3 --kernel-trace --stats -d <dir> -o hip  -- python tools/bench_linear_probe.py --only hip  --epochs 5 --repeats 1 --out ''
    rocprofv3 --kernel-trace --stats -d <dir> -o aten -- python tools/bench_linear_probe.py --only aten --epochs 5 --repeats 1 --out ''
then  python tools/bench_linear_probe.py --stats hip=<hip kernel_stats.csv> aten=<aten kernel_stats.csv> --epochs 5 --repeats 1
merges the counts into the JSON (key "kernel_trace"): --repeats + 1 fits ran in each traced process.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import svm_ref  # noqa: E402  (the synthetic ModelNet40-shaped features)

NCLS, BATCH, WARMUP, BLR = 40, 512, 10, 0.1


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def aten_chain(X, y, Q, yq, weight, order, rates, batch, epochs):
    """The reference's sequence of modules, iteration for iteration; nothing is read back before the end."""
    n, d = X.shape
    ipe = n // batch
    bn = torch.nn.BatchNorm1d(d, affine=False, eps=1e-6).cuda()
    lin = torch.nn.Linear(d, NCLS).cuda()
    with torch.no_grad():
        lin.weight.copy_(weight)
        lin.bias.zero_()
    head = torch.nn.Sequential(bn, lin)
    opt = torch.optim.SGD(lin.parameters(), lr=rates[0], momentum=0.9, weight_decay=0)
    losses, hits = [], []
    t = 0
    for e in range(epochs):
        head.train()
        for it in range(ipe):
            for g in opt.param_groups:
                g["lr"] = rates[t]
            b = order[t * batch:(t + 1) * batch]
            loss = torch.nn.functional.cross_entropy(head(X[b]), y[b])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
            t += 1
        head.eval()
        with torch.no_grad():
            top5 = head(Q).topk(5, dim=1).indices
            hit = top5 == yq.view(-1, 1)
            hits.append(torch.stack([hit[:, 0].sum(), hit.sum()]))
    hits = torch.stack(hits).tolist()                       # the one read
    m = Q.shape[0]
    return [(h[0] * 100.0 / m, h[1] * 100.0 / m) for h in hits], torch.stack(losses)


def timed(fn, repeats):
    out = fn()                                             # warm-up: module load, LDS attribute, allocator, library algorithm choice
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return spread(ts), out


def merge_stats(pairs, fits, iterations, evaluations):
    """kernel_stats.csv of a traced run of one path -> launches and GPU time per training iteration (evaluation kernels included in the
    aten count: its kernels do not say which phase they belong to; the HIP path names its two kernels)."""
    out = {}
    for pair in pairs:
        which, path = pair.split("=", 1)
        rows = list(csv.DictReader(open(path)))
        calls = sum(int(r["Calls"]) for r in rows)
        total = sum(int(r["TotalDurationNs"]) for r in rows)
        entry = {"fits": fits, "iterations_per_fit": iterations, "evaluations_per_fit": evaluations, "kernel_launches": calls,
                 "gpu_time_s": total / 1e9, "launches_per_iteration_all_kernels": calls / (fits * iterations),
                 "top_kernels": [{"name": r["Name"][:100], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
                                 for r in sorted(rows, key=lambda r: -int(r["TotalDurationNs"]))[:6]]}
        for r in rows:
            if "linprobe_train_kernel" in r["Name"]:
                entry["train_launches_per_iteration"] = int(r["Calls"]) / (fits * iterations)
                entry["train_launch_gpu_us"] = {"average": float(r["AverageNs"]) / 1e3, "min": int(r["MinNs"]) / 1e3,
                                                "max": int(r["MaxNs"]) / 1e3}
            if "linprobe_eval_kernel" in r["Name"]:
                entry["eval_launch_gpu_us"] = {"average": float(r["AverageNs"]) / 1e3, "calls": int(r["Calls"])}
        out[which] = entry
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=90)
    ap.add_argument("--only", choices=("hip", "aten"), default=None, help="run one path (for a traced run)")
    ap.add_argument("--stats", nargs="+", default=None, help="hip=<kernel_stats.csv> aten=<kernel_stats.csv>: merge into --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_probe_bench.json"))
    args = ap.parse_args()
    Xtr, ytr, Xte, yte = svm_ref.modelnet40_like(seed=0)
    n, m = len(ytr), len(yte)
    ipe = n // BATCH
    if args.stats:
        with open(args.out) as f:
            res = json.load(f)
        res["kernel_trace"] = merge_stats(args.stats, args.repeats + 1, args.epochs * ipe, args.epochs)
        res["kernel_trace"]["epochs_per_fit"] = args.epochs
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    from gm3d_amd import linear_probe as LP
    from gm3d_amd.data import epoch_order
    X, Q = torch.from_numpy(Xtr + 3.0).cuda(), torch.from_numpy(Xte + 3.0).cuda()      # pooled features sit off zero
    y, yq = torch.from_numpy(ytr).cuda().long(), torch.from_numpy(yte).cuda().long()
    orders = [epoch_order(n, e, True, 0, 0, 1) for e in range(args.epochs)]
    w0 = torch.empty(NCLS, X.shape[1])
    torch.nn.init.trunc_normal_(w0, std=0.01, generator=torch.Generator().manual_seed(0))
    w0 = w0.cuda()
    lr = BLR * BATCH / 256
    warm = min(WARMUP, max(args.epochs - 1, 0))
    rates = LP.learning_rates(args.epochs, ipe, lr, 0.0, warm)
    rates = torch.tensor(rates, dtype=torch.float64).float().tolist()                   # the fp32 values the HIP path holds
    flat = torch.tensor([v for o in orders for v in o[:ipe * BATCH]]).cuda()

    def hip():
        p = LP.LinearProbe(NCLS, batch_size=BATCH, epochs=args.epochs, warmup_epochs=warm, blr=BLR)
        p.fit(X, y, Q, yq, weight=w0, orders=orders)
        return p.history, p.losses

    def aten():
        return aten_chain(X, y, Q, yq, w0, flat, rates, BATCH, args.epochs)

    res = {"device": torch.cuda.get_device_name(0), "shape": {"train": n, "test": m, "classes": NCLS, "d": X.shape[1]},
           "batch": BATCH, "epochs": args.epochs, "warmup_epochs": warm, "iterations": args.epochs * ipe, "peak_lr": lr}
    outs = {}
    for name, fn in (("hip", hip), ("aten", aten)):
        if args.only in (None, name):
            t, (history, losses) = timed(fn, args.repeats)
            outs[name] = losses
            res[name] = {"fit_wall_s": t, "final_top1_top5": list(history[-1]), "max_top1": max(h[0] for h in history),
                         "final_loss": float(losses[-1])}
            print("%-4s fit: %.1f ms wall (%.1f-%.1f), final top-1 / top-5 %s, last loss %.6f"
                  % (name, t["median"] * 1e3, t["min"] * 1e3, t["max"] * 1e3, list(history[-1]), float(losses[-1])))
    if len(outs) == 2:
        res["loss_trajectory_max_abs_difference"] = float((outs["hip"] - outs["aten"]).abs().max())
        res["hip_launches_per_iteration_by_construction"] = (args.epochs * ipe + args.epochs) / (args.epochs * ipe)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

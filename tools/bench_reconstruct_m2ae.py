"""Point-M2AE reconstruction pass: the ragged partition launch beside the aten chain it replaces, and reconstruct_m2ae beside the
forward half of the Point-M2AE step.

Point-M2AE + GeoMask3D (cfgs/config_Point_M2AE.yaml: 512 x 16 / 256 x 8 / 64 x 8, mask ratio 0.8), B = 128 clouds of 2048 points, bf16.
  partition    one ops.reconstruct_partition call against tests/m2ae_reconstruct_ref.partition on the same tensors at the step's two
               shapes -- level 1 (256 x 8, bf16 `rec`) and level 0 (512 x 16, no `pred`) -- with masks from a real pass (both results
               compared with torch.equal first).  Seconds per call over --inner back-to-back calls; the two alternate.
  whole pass   reconstruct_m2ae() per batch (teacher, mask, student in eval mode, loss, two partition launches, two Chamfer
               distances) against the forward half of the training step from the same run: group_stage without augmentation +
               pretrain_forward with gradients recorded, train mode.
--repeats runs of each (median, min, max; one warm-up before).  Writes profiles/reconstruct_m2ae_bench.json and prints it as one JSON
line.  The wall time of a launch is the host's issue rate; the kernel's own time comes from a kernel trace in a run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_reconstruct_m2ae.py --trace-launches 50
  python tools/bench_reconstruct_m2ae.py --kernel-stats DIR/.../*_kernel_stats.csv        # adds the kernel times to the JSON file
Not measured here: runner.test_m2ae's file writing, and anything on more than one GPU.
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

from tests import clouds  # noqa: E402
from tests import m2ae_reconstruct_ref as MR  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12          # bytes/s: a float4 copy on the MI355X, and the HBM3E specification
LEVELS = {"level1": (256, 8, "bf16"), "level0": (512, 16, None)}


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bytes_moved(B, G, k, pred_bytes, n_masked):
    """what one launch has to read and write: every patch once on each side (a masked patch from `pred` when there is one), the
    centres twice, the mask bytes once per 16-token workgroup, order and n_visible"""
    patch = G * k * 3
    read = B * patch * 4 if not pred_bytes else (B * G - n_masked) * k * 3 * 4 + n_masked * k * 3 * pred_bytes
    read += B * G * 3 * 4 + B * ((G + 15) // 16) * G
    return read + B * patch * 4 + B * G * 3 * 4 + B * G * 4 + B * 4


def synthetic(B, G, k, pred, seed=0):
    """the trace run's inputs: random patches, 80 % of the coarse tokens' share masked at random per cloud (ragged)"""
    g = torch.Generator().manual_seed(seed)
    nb, c = (torch.randn(B, G, k, 3, generator=g) * 0.1).cuda(), torch.randn(B, G, 3, generator=g).cuda()
    p = (torch.randn(B, G, 3 * k, generator=g) * 0.1).cuda().bfloat16() if pred else None
    masked = (torch.rand(B, G, generator=g) < (0.55 + 0.2 * torch.rand(B, 1, generator=g))).cuda()
    return p, nb, c, masked


def merge_kernel_stats(path, out):
    """rocprofv3's <pid>_kernel_stats.csv of a --trace-launches run -> the kernel's own time per instantiation, into the JSON file"""
    with open(out) as f:
        res = json.load(f)
    rows = [r for r in csv.DictReader(open(path)) if "reconstruct_partition_kernel" in r["Name"]]
    if not rows:
        raise SystemExit("no reconstruct_partition_kernel in %s" % path)
    res["kernel_trace"] = {}
    for r in rows:
        # <bf16, VEC, PRED> is level 1 (bf16 rec), <float, VEC, no PRED> level 0 (no pred)
        level = "level0" if "float" in r["Name"].split("<", 1)[1].split(",")[0] else "level1"
        t = float(r["AverageNs"]) * 1e-9
        moved = res["partition"][level]["bytes_moved"]
        res["kernel_trace"][level] = {"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_s": t, "min_s": float(r["MinNs"]) * 1e-9,
                                      "max_s": float(r["MaxNs"]) * 1e-9, "bytes_moved": moved, "bytes_per_s": moved / t,
                                      "share_of_measured_hbm_copy_rate": moved / t / HBM_MEASURED,
                                      "share_of_hbm_spec": moved / t / HBM_SPEC}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="reconstruct_m2ae() / forward-half calls per timed run")
    ap.add_argument("--inner", type=int, default=200, help="back-to-back partition calls per timed run")
    ap.add_argument("--trace-launches", type=int, default=0, metavar="N",
                    help="only issue N partition launches at each of the step's two shapes and exit: the program to put behind "
                         "`rocprofv3 --kernel-trace --stats --` for the kernel's own time")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV", help="merge a trace run's kernel_stats.csv into --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct_m2ae_bench.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct_m2ae needs the GPU: nothing here is measured on a CPU")
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import ops
    from gm3d_amd import point_m2ae as P
    from gm3d_amd import reconstruct as RC

    B, N = args.batch, 2048
    if args.trace_launches:
        sets = [synthetic(B, G, k, pred is not None, seed=i) for i, (G, k, pred) in enumerate(LEVELS.values())]
        for _ in range(args.trace_launches):
            for s in sets:
                ops.reconstruct_partition(*s)
        torch.cuda.synchronize()
        print("%d launches issued per level" % args.trace_launches)
        return
    torch.manual_seed(0)
    model = P.PointM2AE().cuda().train()
    ema = E.ModelEma(model, 0.999)
    pts = clouds.gaussian(B, N, seed=1).cuda()
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(2)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16",
           "shape": {"B": B, "N": N, "num_groups": [512, 256, 64], "group_sizes": [16, 8, 8], "mask_ratio": model.mask_ratio},
           "not_measured": ["runner.test_m2ae's file writing", "anything on more than one GPU"]}

    # ---- the whole pass against the forward half of the step
    def whole():
        for _ in range(args.iters):
            r = RC.reconstruct_m2ae(model, pts, ema, 100, 300, mask_noise=noise, bf16=True)
        return r

    def forward_half():
        for _ in range(args.iters):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                _, group, prop = P.group_stage(ema.ema.group_divider, pts, augment=False)
                out = P.pretrain_forward(model, ema.ema, pts, 100, 300, mask_noise=noise, group=group, prop=prop)
        return out
    once(whole), once(forward_half)                        # warm-up: code objects, library algorithm choice, allocator
    wt, ft = [], []
    for _ in range(args.repeats):                          # the two alternate: neither gets the quieter half of the window
        wt.append(once(whole))
        ft.append(once(forward_half))
    res["reconstruct_m2ae"] = {"wall_s_per_batch": spread([t / args.iters for t in wt]),
                               "clouds_per_s": spread([B * args.iters / t for t in wt]), "calls_per_run": args.iters}
    res["step_forward_half"] = {"wall_s_per_batch": spread([t / args.iters for t in ft]), "calls_per_run": args.iters,
                                "what": "group_stage(augment=False) + pretrain_forward, train mode, gradients recorded, eager"}
    res["reconstruct_m2ae"]["over_step_forward_half"] = (res["reconstruct_m2ae"]["wall_s_per_batch"]["median"]
                                                         / res["step_forward_half"]["wall_s_per_batch"]["median"])

    # ---- one partition call against the aten chain, on the tensors of a real pass
    r = whole()
    with torch.no_grad():
        _, group, _ = P.group_stage(ema.ema.group_divider, pts, augment=False)
    res["partition"] = {"calls_per_run": args.inner, "n_visible_level1": {"min": int(r.n_visible.min()), "max": int(r.n_visible.max())},
                        "n_visible_level0": {"min": int(r.n_visible0.min()), "max": int(r.n_visible0.max())}}
    for lvl, name in ((1, "level1"), (0, "level0")):
        nb, c, masked = group[0][lvl], group[1][lvl], r.masks[lvl]
        _, G, k, _ = nb.shape
        assert (G, k) == LEVELS[name][:2]
        pred = r.rec.reshape(B, G, 3 * k) if lvl == 1 else None
        got, want = ops.reconstruct_partition(pred, nb, c, masked), MR.partition(pred, nb, c, masked)
        equal = all(bool(torch.equal(a, b)) for a, b in zip(got, want))

        def launches():
            for _ in range(args.inner):
                ops.reconstruct_partition(pred, nb, c, masked)

        def chains():
            for _ in range(args.inner):
                MR.partition(pred, nb, c, masked)
        lt, ct, ev = [], [], []
        once(launches), once(chains)
        for _ in range(args.repeats):
            lt.append(once(launches))
            ct.append(once(chains))
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launches()
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b) / 1e3 / args.inner)
        moved = bytes_moved(B, G, k, pred.element_size() if pred is not None else 0, int(masked.sum()))
        res["partition"][name] = {"G": G, "k": k, "pred_dtype": str(pred.dtype) if pred is not None else None,
                                  "equal_to_aten_chain": equal, "launch_wall_s_per_call": spread([t / args.inner for t in lt]),
                                  "launch_stream_s_per_call": spread(ev), "aten_chain_wall_s_per_call": spread([t / args.inner for t in ct]),
                                  "bytes_moved": moved}
        res["partition"][name]["aten_over_launch"] = (res["partition"][name]["aten_chain_wall_s_per_call"]["median"]
                                                      / res["partition"][name]["launch_wall_s_per_call"]["median"])
        print("%s partition: %.1f us/call wall (%.1f us back to back on the stream); aten chain: %.1f us/call; equal: %s"
              % (name, res["partition"][name]["launch_wall_s_per_call"]["median"] * 1e6, statistics.median(ev) * 1e6,
                 res["partition"][name]["aten_chain_wall_s_per_call"]["median"] * 1e6, equal))
    print("reconstruct_m2ae(): %.1f ms/batch (%.0f clouds/s); forward half of the step: %.1f ms/batch"
          % (res["reconstruct_m2ae"]["wall_s_per_batch"]["median"] * 1e3, res["reconstruct_m2ae"]["clouds_per_s"]["median"],
             res["step_forward_half"]["wall_s_per_batch"]["median"] * 1e3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

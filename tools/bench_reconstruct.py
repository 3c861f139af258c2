"""Reconstruction pass: gm3d_amd.reconstruct.reconstruct beside the reference's tester restated on the same GPU, and the assemble
launch beside the aten chain it replaces.

Plain Point-MAE (cfgs/config.yaml: 64 groups of 32, mask ratio 0.6, rand), B = 128 clouds of 1024 points, bf16 autocast, eval mode.
  whole pass   reconstruct() on the whole batch with the mask drawn on the device: FPS + KNN, encoder, decoder, patch loss, the
               assemble launch, the Chamfer distance of every dense cloud to its input.  clouds/s.
  reference    what tools/runner.py::test does per cloud, file writing and rendering left out: B = 1 per iteration, the host-drawn
               mask, the forward with its loss, then the boolean-mask indexing of the `vis` branch (models/Point_MAE.py:428-437) and
               the copies of the three clouds to the host.  clouds/s over the same 128 clouds.
  assemble     ops.reconstruct_assemble(flat=True) alone against the aten chain of the `vis` branch at B = 128 on the same tensors
               (both results compared with torch.equal first).  Seconds per call over --inner back-to-back calls.
--repeats runs of each (median, min, max; one warm-up before).  Writes profiles/reconstruct_bench.json and prints it as one JSON line.
The wall time of the launch is the host's issue rate; the kernel's own time comes from a kernel trace in a run of its own:
  rocprofv3 --kernel-trace --stats -- python tools/bench_reconstruct.py --trace-launches 50
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import clouds  # noqa: E402
from tests import point_mae_ref as PR  # noqa: E402


def spread(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "runs": len(ts)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(fn, repeats):
    once(fn)                                               # warm-up: code objects, library algorithm choice, allocator
    return [once(fn) for _ in range(repeats)]


def vis_chain(rebuild_points, neighborhood, center, mask):
    """models/Point_MAE.py:429-437, line for line: rebuild_points (B*M,k,3), mask (B,G) bool."""
    B, G = mask.shape
    M = rebuild_points.shape[0] // B
    vis_points = neighborhood[~mask].reshape(B * (G - M), -1, 3)
    full_vis = vis_points + center[~mask].unsqueeze(1)
    full_rebuild = rebuild_points + center[mask].unsqueeze(1)
    full = torch.cat([full_vis, full_rebuild], dim=0)
    full_center = torch.cat([center[mask], center[~mask]], dim=0)
    ret2 = full_vis.reshape(-1, 3).unsqueeze(0)
    ret1 = full.reshape(-1, 3).unsqueeze(0)
    return ret1, ret2, full_center


@torch.no_grad()
def reference_tester(model, pts):
    """One cloud per iteration, like the reference's test loader (batch size 1)."""
    for i in range(pts.shape[0]):
        p = pts[i:i + 1]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            neighborhood, center, _ = model.group_divider(p)
            mask, _, mask_ids, pred, chosen = model._rebuild(neighborhood, center)          # np.random draw, gathers by id lists
            model._patch_loss(pred, neighborhood, mask_ids, chosen)                          # the forward forms its loss first
            B, M = mask_ids.shape
            ret1, ret2, _ = vis_chain(pred.reshape(B * M, -1, 3), neighborhood, center, mask)
        p.squeeze().cpu().numpy(), ret2.squeeze().cpu().numpy(), ret1.squeeze().cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="reconstruct() calls per timed run")
    ap.add_argument("--inner", type=int, default=200, help="back-to-back assemble calls per timed run")
    ap.add_argument("--trace-launches", type=int, default=0, metavar="N",
                    help="only issue N assemble launches at the benchmark's shape (bf16 pred, flat layout) and exit: the program to put "
                         "behind `rocprofv3 --kernel-trace --stats --` for the kernel's own time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reconstruct needs the GPU: nothing here is measured on a CPU")
    from gm3d_amd import ops
    from gm3d_amd import reconstruct as RC
    from gm3d_amd.models_mae_learn_loss import split_ids
    from gm3d_amd.point_mae import Point_MAE
    from oracle import model_ref as R

    B, N, G, K = args.batch, 1024, 64, 32
    if args.trace_launches:
        g = torch.Generator().manual_seed(0)
        M = int(0.6 * G)
        neighborhood, center = (torch.randn(B, G, K, 3, generator=g) * 0.1).cuda(), torch.randn(B, G, 3, generator=g).cuda()
        pred = (torch.randn(B, M, 3 * K, generator=g) * 0.1).cuda().bfloat16()
        order = torch.stack([torch.randperm(G, generator=g) for _ in range(B)]).cuda()
        for _ in range(args.trace_launches):
            ops.reconstruct_assemble(pred, neighborhood, center, order[:, :G - M], order[:, G - M:], flat=True)
        torch.cuda.synchronize()
        print("%d launches issued" % args.trace_launches)
        return
    torch.manual_seed(0)
    model = R.det_fill_(Point_MAE(PR.config("rand", "cdl2")), seed=41).cuda().eval()
    pts = clouds.gaussian(B, N, seed=1).cuda()
    res = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "N": N, "G": G, "k": K, "mask_ratio": 0.6}, "dtype": "bf16"}

    # ---- the whole pass
    model.MAE_encoder.device_mask = True

    def whole():
        for _ in range(args.iters):
            r = RC.reconstruct(model, pts, bf16=True)
        return r
    ts = timed(whole, args.repeats)
    model.MAE_encoder.device_mask = False
    res["reconstruct"] = {"wall_s_per_call": spread([t / args.iters for t in ts]),
                          "clouds_per_s": spread([B * args.iters / t for t in ts]), "calls_per_run": args.iters}

    # ---- the reference's tester, restated
    ts = timed(lambda: reference_tester(model, pts), args.repeats)
    res["reference_tester"] = {"wall_s_per_cloud": spread([t / B for t in ts]), "clouds_per_s": spread([B / t for t in ts]),
                               "clouds_per_run": B, "left_out": "np.savetxt of the three clouds and the rendered plot.jpg"}
    res["reconstruct"]["speedup_over_reference_tester"] = (res["reconstruct"]["clouds_per_s"]["median"]
                                                           / res["reference_tester"]["clouds_per_s"]["median"])

    # ---- the assemble launch alone against the aten chain of the vis branch
    r = RC.reconstruct(model, pts, mask_noise=torch.rand(B, G, device="cuda"), bf16=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        neighborhood, center, _ = model.group_divider(pts)
    mask, pred = r.mask, r.pred.contiguous()
    M = pred.shape[1]
    vis_ids, mask_ids = split_ids(mask, G - M)
    got = ops.reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=True)
    want = vis_chain(pred.reshape(B * M, -1, 3), neighborhood, center, mask)
    equal = bool(torch.equal(got[0], want[0][0]) and torch.equal(got[1], want[2]))

    def launches():
        for _ in range(args.inner):
            ops.reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=True)

    def chains():
        for _ in range(args.inner):
            vis_chain(pred.reshape(B * M, -1, 3), neighborhood, center, mask)
    lt, ct, ev = [], [], []
    once(launches), once(chains)                           # warm-up
    for _ in range(args.repeats):                          # the two alternate: neither gets the quieter half of the window
        lt.append(once(launches))
        ct.append(once(chains))
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b) / 1e3 / args.inner)
    # bytes the launch reads (visible patches f32, pred, centres) and writes (dense, full_center); the ids are 8 bytes a patch
    moved = (B * (G - M) * K * 3 * 4 + pred.numel() * pred.element_size() + B * G * 3 * 4 + B * G * 8) + (B * G * K * 3 * 4 + B * G * 3 * 4)
    res["assemble"] = {"launch_wall_s_per_call": spread([t / args.inner for t in lt]), "launch_gpu_s_per_call": spread(ev),
                       "aten_chain_wall_s_per_call": spread([t / args.inner for t in ct]), "calls_per_run": args.inner,
                       "equal_to_aten_chain": equal, "pred_dtype": str(pred.dtype), "bytes_moved": moved,
                       "launch_bytes_per_s": moved / statistics.median(ev)}
    res["assemble"]["aten_over_launch"] = (res["assemble"]["aten_chain_wall_s_per_call"]["median"]
                                           / res["assemble"]["launch_wall_s_per_call"]["median"])
    print("reconstruct(): %.0f clouds/s (%.0f-%.0f); reference tester restated: %.0f clouds/s (%.0f-%.0f)"
          % (res["reconstruct"]["clouds_per_s"]["median"], res["reconstruct"]["clouds_per_s"]["min"],
             res["reconstruct"]["clouds_per_s"]["max"], res["reference_tester"]["clouds_per_s"]["median"],
             res["reference_tester"]["clouds_per_s"]["min"], res["reference_tester"]["clouds_per_s"]["max"]))
    print("assemble launch: %.1f us/call wall (%.1f us on the GPU); aten chain: %.1f us/call; equal: %s"
          % (res["assemble"]["launch_wall_s_per_call"]["median"] * 1e6, statistics.median(ev) * 1e6,
             res["assemble"]["aten_chain_wall_s_per_call"]["median"] * 1e6, equal))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

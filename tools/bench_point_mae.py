"""Plain Point-MAE pre-training step (B=128 clouds of 1024 points, G=64, k=32, mask ratio 0.6, bf16) on 1 GPU, three ways in one run:
eager with the reference's host-side mask (the only way to run this step before the device mask existed), eager with the device
mask, and hipGraph replay (engine_pretrain_point_mae.GraphedPointMAEStep).
    python tools/bench_point_mae.py [--batch 128] [--steps 30] [--warmup 5] [--repeats 5]   -> one JSON line
Each mode: --warmup untimed steps, then --repeats timed runs of --steps steps (wall clock around a device synchronisation); the median
run is reported with the min-max spread.  Launches per step: kernel records of one profiled eager step per mode (the replayed graph
launches what the eager device-mask step launches), split into this package's kernels (namespace gm3d) and everything else
(PyTorch's own: aten).  A figure that could not be taken is reported as "not measured"."""
import argparse, json, os, statistics, sys, time
from types import SimpleNamespace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gm3d_amd import engine_pretrain_point_mae as EP
from gm3d_amd.point_mae import Point_MAE
from bench import make_clouds

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--mask-type", default="rand", choices=["rand", "block"])
ap.add_argument("--loss", default="cdl2", choices=["cdl2", "cdl1"])
a = ap.parse_args()

CFG = {"group_size": 32, "num_group": 64, "loss": a.loss,
       "transformer_config": {"mask_ratio": 0.6, "mask_type": a.mask_type, "trans_dim": 384, "encoder_dims": 384, "depth": 12,
                              "drop_path_rate": 0.1, "num_heads": 6, "decoder_depth": 4, "decoder_num_heads": 6}}
args = SimpleNamespace(bf16=True, step_per_update=1)
torch.manual_seed(0)
np.random.seed(0)
model = Point_MAE(CFG).cuda().train()
opt = EP.build_optimizer(model)
pool = [make_clouds(a.batch, 1024, i, "cuda") for i in range(4)]


def host_step(x):
    """the parent's step: Point_MAE.forward with the host shuffle (and its op-chain loss), then the same backward and update."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd.fused import weight_cache
    x = EP.train_transforms(x)
    weight_cache.pin(model)
    weight_cache.refresh()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = model(x)
    E.backward_and_collect(loss, model, opt, None, async_w=False)
    return E.step_update(model, None, opt)


def device_step(x):
    return EP.pretrain_step(model, opt, x, args)["loss"]


def timed(fn):
    for i in range(a.warmup):
        fn(pool[i % 4].clone())
    torch.cuda.synchronize()
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for i in range(a.steps):
            fn(pool[i % 4].clone())
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / a.steps * 1e3)
    med = statistics.median(runs)
    return {"ms_per_step": round(med, 3), "ms_min": round(min(runs), 3), "ms_max": round(max(runs), 3),
            "clouds_per_s": round(a.batch / med * 1e3, 1), "runs": len(runs)}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(pool[0].clone())
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(pool[0].clone())
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name]
        if not names:
            return "not measured"
        ours = sum("gm3d" in n for n in names)
        return {"launches_per_step": len(names), "gm3d": ours, "aten": len(names) - ours, "aten_share": round((len(names) - ours) / len(names), 3)}
    except Exception as e:          # no profiler on this stack
        return "not measured (%s)" % type(e).__name__


res = {"bench": "point_mae_pretrain", "batch": a.batch, "npoints": 1024, "num_group": 64, "group_size": 32, "mask_ratio": 0.6,
       "mask_type": a.mask_type, "loss": a.loss, "dtype": "bf16", "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
model.MAE_encoder.device_mask = False
res["eager_host_mask"] = timed(host_step)
res["eager_host_mask"]["launches"] = launches(host_step)
model.MAE_encoder.device_mask = True
res["eager_device_mask"] = timed(device_step)
res["eager_device_mask"]["launches"] = launches(device_step)
graphed = EP.GraphedPointMAEStep(model, opt, pool[0], args, warmup_iters=0)
res["graph_replay"] = timed(lambda x: graphed(x))
res["graph_replay"]["launches"] = "the eager device-mask step's, as one graph launch"
res["replay_vs_eager_host_mask"] = round(res["eager_host_mask"]["ms_per_step"] / res["graph_replay"]["ms_per_step"], 3)
res["replay_not_slower_than_eager_host_mask"] = res["graph_replay"]["ms_per_step"] <= res["eager_host_mask"]["ms_per_step"]
res["loss_finite"] = bool(torch.isfinite(graphed.out["loss"]))
print(json.dumps(res))

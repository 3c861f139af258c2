"""Point-M2AE + GeoMask3D pretrain step (BASELINE config #4: B=128 clouds of 2048 points, bf16) on 1 GPU: eager and hipGraph replay.
    python tools/bench_m2ae.py [--batch 128] [--steps 20]   -> one JSON line
    --epoch: engine_pretrain_m2ae.train_one_epoch over an in-memory loader of --steps synthetic batches (one warm epoch first: eager
             iterations + capture), timed; --rehearse-gloo: the same with two ranks sharing GPU 0 over gloo (the data-parallel
             SegmentedM2AEStep end to end; the line is marked as a rehearsal, not a measurement)"""
import argparse, json, os, sys, time
from types import SimpleNamespace
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gm3d_amd import engine_pretrain as E, point_m2ae as P
from bench import make_clouds, roofline_of
from gm3d_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--staged", action="store_true", help="A/B: training graph + the next batch's grouping graph on a second stream")
ap.add_argument("--set", action="append", default=[], metavar="mod.ATTR=value",
                help="flip a module switch of gm3d_amd for a same-box A/B (e.g. --set gemm.WS_BN=False --set point_m2ae.VISIBLE_FIRST=False)")
ap.add_argument("--epoch", action="store_true", help="time engine_pretrain_m2ae.train_one_epoch (in-memory loader of --steps batches)")
ap.add_argument("--rehearse-gloo", action="store_true", help="--epoch with two ranks on GPU 0 over gloo (a rehearsal, not a measurement)")
a = ap.parse_args()
if a.rehearse_gloo and "RANK" not in os.environ:      # the launcher: two fresh rank processes of this script, rank 0's line
    import socket, subprocess
    with socket.socket() as _s:
        _s.bind(("127.0.0.1", 0))
        port = _s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], stdout=subprocess.PIPE, text=True,
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for r in range(2)]
    outs, rcs = [], []
    try:
        for p_ in procs:
            outs.append(p_.communicate(timeout=1500)[0])
            rcs.append(p_.returncode)
    finally:
        for p_ in procs:
            if p_.poll() is None:
                p_.kill()
                p_.wait()
    lines = [l for l in (outs[0] if outs else "").splitlines() if l.startswith("{")]
    if rcs != [0, 0] or not lines:
        sys.exit("rank exit codes %s" % rcs)
    print(lines[-1])
    sys.exit(0)
import importlib
for item in a.set:
    name, val = item.split("=")
    mod, attr = name.rsplit(".", 1)
    setattr(importlib.import_module("gm3d_amd." + mod), attr, eval(val))


def epoch_bench():
    """train_one_epoch, warm epoch then timed epoch; one JSON line (rank 0)."""
    from gm3d_amd import engine_pretrain_m2ae as EM
    rank, world = 0, 1
    if "RANK" in os.environ:
        import torch.distributed as dist
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(rank)
    model = P.PointM2AE().cuda().train()
    opt, ema = EM.build_optimizer(model, lr=1e-3)
    args = SimpleNamespace(bf16=True, epochs=300, lr=1e-3, min_lr=1e-6, warmup_epochs=10, accum_iter=1, seed=0)
    loader = [make_clouds(a.batch, 2048, 100 + i + 1000 * rank, "cuda") for i in range(a.steps)]
    warm = EM.train_one_epoch(model, loader[:E.EAGER_WARMUP_ITERS + a.warmup], opt, "cuda", 99, args=args, model_ema=ema, print_freq=10 ** 6)
    st = EM.train_one_epoch(model, loader, opt, "cuda", 100, args=args, model_ema=ema, print_freq=10 ** 6)
    line = {"metric": "point-clouds/sec Point-M2AE+GM3D train_one_epoch (N=2048, G=512/256/64)", "unit": "clouds/s", "n_gpus": 1,
            "ranks": world, "dtype": "bf16", "data": "synthetic, in-memory loader", "batch_per_rank": a.batch, "iters": a.steps,
            "value": st["replay_clouds_per_s"], "epoch_clouds_per_s": st["clouds_per_s"], "replayed_iters": st["replayed_iters"],
            "capture_s": st["capture_s"], "warm_epoch_eager_iters": E.EAGER_WARMUP_ITERS + a.warmup - warm["replayed_iters"],
            "loss": st["loss"] + st["loss_learn"],
            "execution": "GraphedM2AEStep replays, look-ahead grouping" if world == 1 else
                         "SegmentedM2AEStep: 6 graphs, 4 segment all-reduces per step"}
    if world > 1:
        line["rehearsal"] = "%d gloo ranks sharing GPU 0: the data-parallel code path, not a measurement" % world
    if rank == 0:
        print(json.dumps(line))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if a.epoch or a.rehearse_gloo:
    epoch_bench()
    sys.exit(0)
# (no TunableOp table: since round 4 every product of this step runs on a hand-written kernel -- rocprof: 0 library launches)
torch.manual_seed(0)
model = P.PointM2AE().cuda().train()
ema = E.ModelEma(model, 0.999)
opt = E.build_optimizer(model, lr=1e-3, flat=True, model_ema=ema)
args = SimpleNamespace(bf16=True, epochs=300)
pool = [make_clouds(a.batch, 2048, 100 + i, "cuda") for i in range(4)]


def run(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        o = step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, o


eager = lambda i: P.pretrain_step(model, ema, opt, pool[i % 4].clone(), 100, args)
run(eager, a.warmup)
t_eager, o = run(eager, a.steps)
line = {"metric": "point-clouds/sec Point-M2AE+GM3D pretrain step (N=2048, G=512/256/64)", "unit": "clouds/s", "n_gpus": 1,
        "dtype": "bf16", "data": "synthetic", "batch": a.batch, "eager_ms_per_step": t_eager * 1e3, "eager_clouds_per_s": a.batch / t_eager,
        "loss": float(o["loss"])}
try:
    if not a.staged:          # the whole step as ONE graph (grouping in line): what bench.py's secondary leg runs
        static_in = pool[0].clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = P.pretrain_step(model, ema, opt, static_in, 100, args)

        def replay(i):
            static_in.copy_(pool[i % 4])
            g.replay()
            return out
    else:                     # training graph + the next batch's grouping graph on a second stream (point_m2ae.GraphedM2AEStep)
        gs = P.GraphedM2AEStep(model, ema, opt, args, pool[0], 100)
        replay = lambda i: gs(pool[i % 4], next_pts=pool[(i + 1) % 4])
    run(replay, a.warmup)
    t_graph, o = run(replay, a.steps)
    gl = float(o["loss"])
    if gl != gl or abs(gl) == float("inf"):     # this model still runs PyTorch reductions that are not replay-safe on this stack
        raise RuntimeError("replayed loss is not finite (torch multi-block reductions under replay: DESIGN 3c)")
    line.update(graph_ms_per_step=t_graph * 1e3, value=a.batch / t_graph, ms_per_step=t_graph * 1e3, graph_loss=gl,
                execution="hipGraph replay")
except Exception as ex:
    line.update(value=a.batch / t_eager, ms_per_step=t_eager * 1e3, execution="eager (capture failed: %s)" % str(ex)[:100])
# per-kernel rooflines of the hand-written kernels (HIP events around every launch of two eager steps): the masked attention's
# fraction of the bf16 MFMA peak (dense flop count: blocked pairs are computed too) and the GEMM families'
probe = ops.KernelTimer()
ops.set_kernel_timer(probe)
for i in range(2):
    eager(i)
ops.set_kernel_timer(None)
roof = {}
for n, v in probe.summary().items():
    q = roofline_of(n, v["per_launch"], v["total_ms"])
    if q is None:
        continue
    roof[n] = {"bound": q["bound"], "achieved": round(q["achieved"], 2), "unit": q["unit"], "frac": round(q["frac"], 4),
               "launches_per_step": v["launches"] / 2, "ms_per_step": round(v["total_ms"] / 2, 3)}
    for k in ("tflops", "frac_mfma", "gbs", "frac_hbm"):
        if k in q:
            roof[n][k] = q[k]
line["kernel_rooflines"] = dict(sorted(roof.items(), key=lambda kv: -kv[1]["ms_per_step"])[:10])
print(json.dumps(line))

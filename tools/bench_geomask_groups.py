"""The GeoMask3D pretrain step at num_group 64 / 128 / 256 / 512 (bf16, clouds of 1024 points for 64, 2048 / 4096 / 8192 above so
that every group keeps its 32 points' worth of cloud), eager and replayed from the captured graph, and each launch of csrc/guided.hip
against the aten chain it replaces, on the same tensors: the guided mask + id lists (generate_mask_ids vs two argsorts, two scatters,
the bool cast and split_ids' argsort) and the ranking loss forward + backward (heads.rank_loss_tail vs the (B,M,M) broadcast chain).
B = 128 where it fits, else the largest power of two that does (stated per row).  HIP events around a train of steps / launches; five
runs each: median with min-max.
python tools/bench_geomask_groups.py [--json profiles/geomask_groups_bench.json] [--batch 128] [--groups 64,128,256,512]"""
import gc, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace
from gm3d_amd import engine_pretrain as E, heads, models_mae_learn_loss as M
from bench import make_clouds

dev = torch.device("cuda")
RUNS, EPOCH, RATIO = 5, 200, 0.6
POINTS = {64: 1024, 128: 2048, 256: 4096, 512: 8192}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"median": statistics.median(out), "min": min(out), "max": max(out), "runs": len(out)}


def step_times(G, B):
    """eager and replayed step, ms; the model is freed before returning"""
    args = SimpleNamespace(mask_ratio=RATIO, epochs=400, relative=True, bf16=True, accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=40)
    torch.manual_seed(0)
    model = M.mae_vit_base_patch16_dec512d8b(num_group=G).to(dev).train()
    ema = E.ModelEma(model, decay=E.ema_decay_for_epoch(EPOCH))
    opt = E.build_optimizer(model, lr=1e-3, weight_decay=0.05, flat=True, model_ema=ema)
    torch.manual_seed(1234)
    pool = [make_clouds(B, POINTS.get(G, 16 * G), 1234 + 1000 * i, dev) for i in range(2)]
    it = [0]

    def eager():
        it[0] += 1
        E.pretrain_step(model, ema, opt, pool[it[0] % 2].clone(), EPOCH, args)

    res = {"eager_ms": timed(eager, 4, warm=3)}
    graphed = E.GraphedPretrainStep(model, ema, opt, args, pool[0], EPOCH, warmup_iters=0)

    def replay():
        it[0] += 1
        graphed(pool[it[0] % 2])

    res["replay_ms"] = timed(replay, 8, warm=3)
    res["loss_chfr_last"] = float(graphed.out["loss_chfr"])
    res["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    del graphed, opt, ema, model, pool
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    return res


def aten_mask(lp, noise, len_keep, len_loss):
    """what engine_pretrain / reconstruct run above the kernels' limit: generate_mask's aten formulation, the bool cast, split_ids"""
    L = lp.shape[1]
    nz = noise.clone()
    if len_loss > 0:
        nz.scatter_(1, torch.argsort(lp, dim=1)[:, L - len_loss:], float("inf"))
    mask = torch.ones_like(lp)
    mask.scatter_(1, torch.argsort(nz, dim=1)[:, :len_keep], 0.0)
    mb = mask.to(torch.bool)
    return (mask, mb) + M.split_ids(mb, len_keep)


def aten_rank(p, t):
    pos, neg = t.unsqueeze(1) > t.unsqueeze(2), t.unsqueeze(1) < t.unsqueeze(2)
    sig = torch.sigmoid(p.unsqueeze(1) - p.unsqueeze(2))
    loss = -pos.to(sig.dtype) * torch.log(sig + 1e-6) - neg.to(sig.dtype) * torch.log(1 - sig + 1e-6)
    return loss.sum() / (pos | neg).sum()


def launch_times(G, B):
    g = torch.Generator().manual_seed(G)
    lp, noise = torch.randn(B, G, generator=g).to(dev), torch.rand(B, G, generator=g).to(dev)
    len_keep = int(G * (1 - RATIO))
    len_loss = int((G - len_keep) * (float((EPOCH + 1) / 400) * 0.5))
    Mm = G - len_keep
    res = {"mask_ours_ms": timed(lambda: M.generate_mask_ids(lp, RATIO, True, EPOCH, 400, noise, want_bool=True), 200),
           "mask_aten_ms": timed(lambda: aten_mask(lp, noise, len_keep, len_loss), 50)}
    a, b = M.generate_mask_ids(lp, RATIO, True, EPOCH, 400, noise, want_bool=True), aten_mask(lp, noise, len_keep, len_loss)
    res["mask_equal"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[2]) and torch.equal(a[2], b[3]))
    full = torch.randn(B, G, generator=g).to(dev).requires_grad_(True)
    target = torch.rand(B, Mm, generator=g).to(dev)

    def ours():
        full.grad = None
        heads.rank_loss_tail(full, Mm, target).backward()

    def aten():
        full.grad = None
        aten_rank(full[:, -Mm:], target).backward()

    res["rank_M"] = Mm
    res["rank_ours_fwd_bwd_ms"] = timed(ours, 200)
    res["rank_aten_fwd_bwd_ms"] = timed(aten, 20)
    with torch.no_grad():
        res["rank_rel_diff"] = float((heads.rank_loss_tail(full, Mm, target) / aten_rank(full[:, -Mm:], target) - 1).abs())
    return res


if __name__ == "__main__":
    want_B = int(arg("--batch", 128))
    groups = [int(x) for x in arg("--groups", "64,128,256,512").split(",")]
    res = {"unit": "ms per step / per launch train (median, min, max of %d runs)" % RUNS, "dtype": "bf16", "epoch": EPOCH, "mask_ratio": RATIO,
           "device": torch.cuda.get_device_name(0), "rows": []}
    fmt = lambda r: "%9.3f (%.3f-%.3f)" % (r["median"], r["min"], r["max"])
    for G in groups:
        B = want_B
        while True:
            try:
                row = {"num_group": G, "points": POINTS.get(G, 16 * G), "B": B, **step_times(G, B)}
                break
            except torch.OutOfMemoryError:
                gc.collect(); torch.cuda.empty_cache()
                if B == 1:
                    raise
                B //= 2
        row.update(launch_times(G, B))
        res["rows"].append(row)
        print("G=%3d N=%4d B=%3d  step eager %s  replay %s ms | mask ours %s aten %s | rank(M=%d) ours %s aten %s" % (
            G, row["points"], B, fmt(row["eager_ms"]), fmt(row["replay_ms"]), fmt(row["mask_ours_ms"]), fmt(row["mask_aten_ms"]),
            row["rank_M"], fmt(row["rank_ours_fwd_bwd_ms"]), fmt(row["rank_aten_fwd_bwd_ms"])), flush=True)
    path = arg("--json", None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", path)

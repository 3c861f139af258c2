"""The pre-training steps at the reference's three geometries -- 64 groups x 32 points, 128 x 16, 256 x 8, clouds of 1024 points, bf16,
B = 128 -- and the fused masked-patch loss for 16- and 8-point patches against the op chain it replaces:
  * GeoMask3D step (mask ratio 0.6), eager and replayed from the captured graph;
  * plain Point-MAE step (mask ratio 0.6 / 0.75 / 0.6 as config.yaml / config_2 / config_3 have it), replayed;
  * heads.PatchChamferLossFn forward + backward vs gather + cast + ops.chamfer + two means and their autograd backward, on the same
    tensors (B x M patches as the GeoMask3D step has them: 128 x 77 at k = 16, 128 x 154 at k = 8), f32 and bf16 predictions.
HIP events around a train of steps / calls; five runs each: median with min-max.  The loss rows time the Python wrappers with the
launches (that is how the step pays for them); kernel-only times are not measured here.
python tools/bench_group_size.py [--json profiles/group_size_bench.json] [--batch 128]"""
import gc, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from types import SimpleNamespace
from gm3d_amd import engine_pretrain as E, engine_pretrain_point_mae as EP, heads, models_mae_learn_loss as M, ops
from gm3d_amd.point_mae import Point_MAE
from bench import make_clouds

dev = torch.device("cuda")
RUNS, EPOCH = 5, 200
GEOMETRIES = ((64, 32, 0.6), (128, 16, 0.75), (256, 8, 0.6))      # num_group, group_size, plain Point-MAE's mask ratio in the reference's config


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


def free():
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()


def geomask_times(G, k, B):
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=40)
    torch.manual_seed(0)
    model = M.mae_vit_base_patch16_dec512d8b(num_group=G, group_size=k).to(dev).train()
    ema = E.ModelEma(model, decay=E.ema_decay_for_epoch(EPOCH))
    opt = E.build_optimizer(model, lr=1e-3, weight_decay=0.05, flat=True, model_ema=ema)
    pool = [make_clouds(B, 1024, 1234 + 1000 * i, dev) for i in range(2)]
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
    free()
    return res


def point_mae_times(G, k, ratio, B):
    cfg = {"group_size": k, "num_group": G, "loss": "cdl2",
           "transformer_config": {"mask_ratio": ratio, "mask_type": "rand", "trans_dim": 384, "encoder_dims": 384, "depth": 12,
                                  "drop_path_rate": 0.1, "num_heads": 6, "decoder_depth": 4, "decoder_num_heads": 6}}
    args = SimpleNamespace(bf16=True, step_per_update=1)
    torch.manual_seed(0)
    model = Point_MAE(cfg).to(dev).train()
    model.MAE_encoder.device_mask = True
    opt = EP.build_optimizer(model)
    pool = [make_clouds(B, 1024, 99 + 1000 * i, dev) for i in range(2)]
    for i in range(3):
        EP.pretrain_step(model, opt, pool[i % 2].clone(), args)
    graphed = EP.GraphedPointMAEStep(model, opt, pool[0], args, warmup_iters=0)
    it = [0]

    def replay():
        it[0] += 1
        graphed(pool[it[0] % 2])

    res = {"mask_ratio": ratio, "replay_ms": timed(replay, 8, warm=3), "loss_last": float(graphed.out["loss"])}
    del graphed, opt, model, pool
    free()
    return res


def loss_times(k, B, Mm, dtype):
    """fused forward + backward vs the chain of forward_loss without it, both from the batch-strided last-Mm slice of a (B,G,3k) head
    output and the id list"""
    G = Mm * 5 // 3 + 1
    g = torch.Generator().manual_seed(k)
    pix = (torch.randn(B, G, 3 * k, generator=g) * 0.3).to(dev).to(dtype).requires_grad_(True)
    target = (torch.randn(B, G, k, 3, generator=g) * 0.3).to(dev)
    ids = torch.stack([torch.randperm(G, generator=g) for _ in range(B)]).to(dev)[:, G - Mm:]
    assert heads.patch_chamfer_loss_supported(pix[:, G - Mm:], target, ids)

    def fused():
        pix.grad = None
        heads.PatchChamferLossFn.apply(pix, target, ids, True)[0].backward()

    def chain():
        pix.grad = None
        tg = M.take(target, ids).reshape(-1, k, 3).to(torch.float32)
        pr = pix[:, G - Mm:].reshape(-1, k, 3).to(torch.float32)
        ops.ChamferDistanceL2()(pr, tg).reshape(B, -1, k).mean(dim=-1).mean().backward()

    fused(); a = pix.grad.clone()
    chain(); b = pix.grad.clone()
    scale = float(b.float().abs().max())
    return {"k": k, "B": B, "M": Mm, "dtype": str(dtype).replace("torch.", ""), "fused_fwd_bwd_ms": timed(fused, 200, warm=50),
            "chain_fwd_bwd_ms": timed(chain, 100, warm=50), "grad_max_diff_over_max": float((a.float() - b.float()).abs().max()) / scale}


if __name__ == "__main__":
    B = int(arg("--batch", 128))
    res = {"unit": "ms per step / per forward + backward (median, min, max of %d runs)" % RUNS, "dtype": "bf16", "epoch": EPOCH, "B": B,
           "points": 1024, "device": torch.cuda.get_device_name(0), "geomask3d": [], "point_mae": [], "patch_loss": [],
           "not_measured": "kernel-only times, other batch sizes, multi-GPU"}
    fmt = lambda r: "%8.3f (%.3f-%.3f)" % (r["median"], r["min"], r["max"])
    for k, Mm in ((16, 77), (8, 154)):
        for dtype in (torch.bfloat16, torch.float32):
            row = loss_times(k, B, Mm, dtype)
            res["patch_loss"].append(row)
            print("patch loss k=%2d B=%d M=%3d %-8s fused %s chain %s ms, grad diff %.2e of max" % (
                k, B, Mm, row["dtype"], fmt(row["fused_fwd_bwd_ms"]), fmt(row["chain_fwd_bwd_ms"]), row["grad_max_diff_over_max"]), flush=True)
    for G, k, ratio in GEOMETRIES:
        row = {"num_group": G, "group_size": k, **geomask_times(G, k, B)}
        row["replay_clouds_per_s"] = B / row["replay_ms"]["median"] * 1e3
        res["geomask3d"].append(row)
        prow = {"num_group": G, "group_size": k, **point_mae_times(G, k, ratio, B)}
        prow["replay_clouds_per_s"] = B / prow["replay_ms"]["median"] * 1e3
        res["point_mae"].append(prow)
        print("%3d x %2d  GeoMask3D eager %s replay %s ms | Point-MAE (ratio %.2f) replay %s ms" % (
            G, k, fmt(row["eager_ms"]), fmt(row["replay_ms"]), ratio, fmt(prow["replay_ms"])), flush=True)
    path = arg("--json", None)
    if path:
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", path)

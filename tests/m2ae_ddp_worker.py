"""One rank of the two-rank Point-M2AE data-parallel test (tests/test_gpu_m2ae_ddp.py): both ranks share cuda:0, backend gloo.

    python -m tests.m2ae_ddp_worker --rank R --world 2 --port P --out DIR

Per mode (SegmentedM2AEStep eager, then hipGraph-captured) the rank writes DIR/<mode>_rank<R>.pt with:
  p_start   flat parameters right after construction (the ranks were seeded differently: rank 0's broadcast must win)
  g_local   flat gradient of this rank's shard alone (the four segments run eagerly without collectives, nothing updated)
  g_avg     flat gradient after the four collectives of step 1
  params / ema   flat parameters / teacher after 3 steps;  losses per step
and DIR/epoch_rank<R>.pt: engine_pretrain_m2ae.train_one_epoch with world 2 for one short epoch (3 eager iterations, capture,
2 replays).  Errors go to DIR/error_rank<R>.txt.
"""
import argparse
import os
import sys
import traceback
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _model(seed):
    import torch
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(seed)
    m = P.PointM2AE().cuda().train()
    for mod in m.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
    opt, ema = EM.build_optimizer(m, lr=1e-3, segmented=True)
    return m, ema, opt


def run(rank, world, port, out, B=4, steps=3):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import point_m2ae as P
    from tests import clouds
    args = SimpleNamespace(bf16=True, epochs=300, lr=1e-3, min_lr=1e-6, warmup_epochs=10, accum_iter=1, seed=0)
    data = [clouds.gaussian(B * world, 2048, 500 + i) for i in range(steps + 1)]
    noise = [torch.rand(B * world, 64, generator=torch.Generator().manual_seed(600 + i)) for i in range(steps + 1)]
    ids = E.shard_for_rank(B * world, rank, world, shuffle=False)
    shard = lambda i: data[i][ids].cuda()
    for mode in ("eager", "graph"):
        m, ema, opt = _model(100 + rank)                     # rank-dependent initial weights
        eager = P.SegmentedM2AEStep(m, ema, opt, args, shard(0), 100, augment=False, inject_mask_noise=True, use_graphs=False)
        p_start = opt.P.clone()
        # this rank's shard alone, eagerly in both modes: the four segments without their collectives
        bufs = [t.detach().clone() for t in m.buffers()]
        eager.static_noise.copy_(noise[0][ids].cuda())
        staged = P.group_stage(ema.ema.group_divider, shard(0), augment=False)
        for k in range(4):
            eager._segment(k, staged if k == 0 else None)
        eager._cuts = eager._grads = None
        with torch.no_grad():                               # the extra forward moved the BatchNorm running statistics: roll back
            for t, v in zip(m.buffers(), bufs):
                t.copy_(v)
        torch.cuda.synchronize()
        g_local = opt.G.clone()
        step = eager if mode == "eager" else P.SegmentedM2AEStep(m, ema, opt, args, shard(0), 100, augment=False, inject_mask_noise=True,
                                                                  warmup_iters=0, broadcast=False)
        losses, g_avg = [], None
        for i in range(steps):
            o = step(shard(i), mask_noise=noise[i][ids].cuda())
            torch.cuda.synchronize()
            if i == 0:
                g_avg = opt.G.clone()
            losses.append([float(o["loss_chfr"]), float(o["loss_learn"]), float(o["grad_norm"])])
        torch.save({"p_start": p_start.cpu(), "g_local": g_local.cpu(), "g_avg": g_avg.cpu(), "params": opt.P.cpu(), "ema": opt.E.cpu(),
                    "losses": losses, "segments": {k: list(v) for k, v in opt.segment_ranges.items()}},
                   os.path.join(out, "%s_rank%d.pt" % (mode, rank)))
        del step, eager, opt, ema, m
    # the engine with world 2: one short epoch (augmentation and DropPath on, per-rank generators)
    torch.manual_seed(200 + rank)
    m = P.PointM2AE().cuda().train()
    opt, ema = EM.build_optimizer(m, lr=1e-3)              # segmented by default: a group of 2 is alive
    loader = [clouds.gaussian(B, 2048, 700 + 10 * rank + i) for i in range(5)]
    stats = EM.train_one_epoch(m, loader, opt, "cuda", 0, args=args, model_ema=ema, print_freq=5)
    torch.cuda.synchronize()
    torch.save({"stats": stats, "params": opt.P.cpu(), "ema": opt.E.cpu()}, os.path.join(out, "epoch_rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    try:
        run(a.rank, a.world, a.port, a.out)
    except Exception:
        with open(os.path.join(a.out, "error_rank%d.txt" % a.rank), "w") as f:
            f.write(traceback.format_exc())
        sys.exit(1)


if __name__ == "__main__":
    main()

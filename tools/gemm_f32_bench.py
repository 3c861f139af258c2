"""fp32 MFMA GEMMs (csrc/gemm_f32.hip) vs the BLAS library (torch.mm / torch.bmm in fp32) on the fp32 step's shapes -- captured trains
of launches timed with HIP events, as tools/gemm_kbench.py -- and the eager fp32 GeoMask3D step at B = 16 with gemm.F32_OWN on / off.
Five runs each: median with min-max.
python tools/gemm_f32_bench.py [--json profiles/gemm_f32_bench.json] [--no-step]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gm3d_amd import gemm

dev = torch.device("cuda")
RUNS = 5
# (M, K, N): forward and input-gradient products of the blocks at B = 128 tokens x 64 (8192 rows), of the mini-PointNet over the point
# rows at B = 16 (32,768 rows) and of the heads
TN = [(8192, 384, 1536), (8192, 1536, 384), (8192, 384, 1152), (8192, 1152, 384), (8192, 384, 384),
      (32768, 128, 256), (32768, 256, 512), (32768, 512, 384), (32768, 384, 512), (1024, 384, 1024), (1024, 128, 384), (1024, 384, 96)]
# (batch, R, N, K): weight gradients of a 12-block stack, of a 4-block decoder, of the mini-PointNet and of a head
NT = [(12, 8192, 1536, 384), (12, 8192, 384, 1536), (12, 8192, 1152, 384), (4, 8192, 384, 384), (1, 32768, 512, 256), (1, 32768, 384, 512),
      (1, 1024, 1024, 384)]


def train(fn, sets, iters=20):
    for s in sets:
        fn(*s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for i in range(iters):
                fn(*sets[i % len(sets)])
    torch.cuda.synchronize()
    g.replay(); torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); g.replay(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def step_ms(on, B=16, iters=6):
    from types import SimpleNamespace
    from gm3d_amd import engine_pretrain as E, models_mae_learn_loss as M
    from bench import make_clouds
    gemm.F32_OWN = on
    try:
        torch.manual_seed(0)
        m = M.mae_vit_base_patch16_dec512d8b().to(dev).train()
        ema = E.ModelEma(m, 0.9999)
        opt = E.build_optimizer(m, lr=1e-3, weight_decay=0.05, flat=True, model_ema=ema)
        args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=False, accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=40)
        x = make_clouds(B, 1024, 1, dev)
        for _ in range(3):
            E.pretrain_step(m, ema, opt, x.clone(), 200, args)
        out = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                E.pretrain_step(m, ema, opt, x.clone(), 200, args)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / iters)
        return out
    finally:
        gemm.F32_OWN = False


if __name__ == "__main__":
    res = {"unit": "us per launch (kernels), ms per step (step)", "tn": [], "nt": [], "step_b16_eager_fp32": {}}
    for M, K, N in TN:
        sets = [(torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5, torch.empty(M, N, device=dev)) for _ in range(3)]
        own = stat(train(lambda x, w, o: gemm.linear_tn_f32(x, w, None, o), sets))
        lib = stat(train(lambda x, w, o: torch.mm(x, w.t(), out=o), sets))
        fl = 2.0 * M * K * N
        res["tn"].append({"M": M, "K": K, "N": N, "own_us": own, "lib_us": lib})
        print("TN M=%6d K=%4d N=%4d  own %7.1f us (%.1f-%.1f) = %5.1f TF/s | lib %7.1f us (%.1f-%.1f) | own / lib x%.2f"
              % (M, K, N, own["median"], own["min"], own["max"], fl / own["median"] / 1e6, lib["median"], lib["min"], lib["max"],
                 own["median"] / lib["median"]), flush=True)
    for nb, R, N, K in NT:
        sets = [(torch.randn(nb, R, N, device=dev), torch.randn(nb, R, K, device=dev), torch.empty(nb, N, K, device=dev)) for _ in range(2)]
        own = stat(train(lambda dy, x, o: gemm.wgrad_nt_f32(dy, x, o), sets))
        lib = stat(train(lambda dy, x, o: torch.bmm(dy.transpose(1, 2), x, out=o), sets))
        fl = 2.0 * nb * R * N * K
        res["nt"].append({"batch": nb, "R": R, "N": N, "K": K, "splits": gemm.nt_f32_splits(nb, R, N, K), "own_us": own, "lib_us": lib})
        print("NT b=%2d R=%6d N=%4d K=%4d  own %7.1f us (%.1f-%.1f) = %5.1f TF/s | lib %7.1f us (%.1f-%.1f) | own / lib x%.2f"
              % (nb, R, N, K, own["median"], own["min"], own["max"], fl / own["median"] / 1e6, lib["median"], lib["min"], lib["max"],
                 own["median"] / lib["median"]), flush=True)
    if "--no-step" not in sys.argv:
        for on in (False, True):
            s = stat(step_ms(on))
            res["step_b16_eager_fp32"]["F32_OWN=%s" % on] = s
            print("eager fp32 GeoMask3D step, B = 16, F32_OWN=%s: %.2f ms (%.2f-%.2f)" % (on, s["median"], s["min"], s["max"]), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", path)

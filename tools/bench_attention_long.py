"""Streaming attention (csrc/attention_long.hip, 513 <= T <= 2048) against an aten softmax(Q K^T) V chain on the same GPU, forward
and backward, T = 513 / 1024 / 2048 at B = 32, H = 6, hd = 64, both dtypes.  There is no earlier time of our own to compare with:
before these kernels the shapes were refused.  HIP events around a train of launches; five runs each: median with min-max.
python tools/bench_attention_long.py [--json profiles/attention_long_bench.json]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gm3d_amd import ops
from gm3d_amd._capi import check, lib

dev = torch.device("cuda")
RUNS, B, H, HD = 5, 32, 6, 64
SCALE = HD ** -0.5


def timed(fn, iters):
    fn(); fn()
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


def aten_forward(qkv):
    q, k, v = qkv.view(B, -1, 3, H, HD).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-2, -1)) * SCALE).softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, -1, H * HD)


def bench(T, dtype):
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B, T, 3 * H * HD, generator=g).to(dtype).to(dev)
    dout = torch.randn(B, T, H * HD, generator=g).to(dtype).to(dev)
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=dev)
    dt = ops._DT[dtype]
    iters = 10 if dtype == torch.bfloat16 else 2

    def fwd():
        check(lib.gm3d_attention_long_fwd(ops._ptr(qkv), None, ops._ptr(out), ops._ptr(lse), B, T, H, HD, SCALE, dt, ops._stream()), "fwd")

    def bwd():
        check(lib.gm3d_attention_long_bwd(ops._ptr(qkv), None, ops._ptr(out), ops._ptr(dout), ops._ptr(lse), ops._ptr(dqkv), B, T, H, HD,
                                          SCALE, dt, ops._stream()), "bwd")

    res = {"T": T, "dtype": str(dtype).replace("torch.", ""), "ours_fwd_ms": timed(fwd, iters), "ours_bwd_ms": timed(bwd, iters)}
    with torch.no_grad():
        res["aten_fwd_ms"] = timed(lambda: aten_forward(qkv), iters)
    x = qkv.clone().requires_grad_(True)
    y = aten_forward(x)
    res["aten_bwd_ms"] = timed(lambda: torch.autograd.grad(y, x, dout, retain_graph=True), iters)
    # the two sides compute the same thing (a sanity line, not a test: tests/test_gpu_attention_long.py holds the kernels to fp64)
    res["max_abs_diff_out"] = float((out.float() - y.detach().float()).abs().max())
    return res


if __name__ == "__main__":
    res = {"unit": "ms per launch (ours) / per chain (aten)", "shape": {"B": B, "H": H, "hd": HD}, "device": torch.cuda.get_device_name(0),
           "rows": []}
    for dtype in (torch.bfloat16, torch.float32):
        for T in (513, 1024, 2048):
            r = bench(T, dtype)
            res["rows"].append(r)
            print("%-8s T=%4d  fwd ours %8.3f ms (%.3f-%.3f) | aten %8.3f ms (%.3f-%.3f)   bwd ours %8.3f ms (%.3f-%.3f) | aten %8.3f ms "
                  "(%.3f-%.3f)" % (r["dtype"], T, *(r[k][s] for k in ("ours_fwd_ms", "aten_fwd_ms", "ours_bwd_ms", "aten_bwd_ms")
                                                   for s in ("median", "min", "max"))), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", path)

"""Weight-gradient (NT) GEMM: hand-written kernel (csrc/gemm_nt.hip) vs the library path (torch.bmm -> hipBLASLt)
at the step's shapes.  python tools/wgrad_bench.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gm3d_amd import gemm

dev = torch.device("cuda")


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(iters):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (2 * iters)


def big_splits(nb, R, N, K):
    """row splits for the 128 x 384-tile kernel (one 512-thread workgroup per CU): the smallest split that offers >= 224 workgroups
    while every split keeps >= 256 rows (8 stages)"""
    tiles, s = nb * (N // 128) * (K // 384), 1
    while tiles * s < 224 and s < 64 and R % (64 * s) == 0 and R // (2 * s) >= 256:
        s *= 2
    return s


shapes = [(12, 3200, 384, 1536), (12, 3200, 1536, 384), (12, 3200, 384, 384), (12, 3200, 1152, 384),
          (4, 8192, 384, 1536), (4, 8192, 1536, 384), (4, 8192, 384, 384), (4, 8192, 1152, 384),
          (1, 262144, 256, 128), (1, 262144, 512, 256), (1, 102400, 384, 512), (1, 8192, 512, 256), (1, 8192, 1024, 384)]
if __name__ == "__main__":
  print("%-28s %10s %10s %8s   splits" % ("(nb, R, N, K)", "own us", "library us", "ratio"))
  lib_ = __import__("gm3d_amd._capi", fromlist=["lib"]).lib
  for nb, R, N, K in shapes:
      dy = torch.randn(nb, R, N, device=dev).bfloat16()
      x = torch.randn(nb, R, K, device=dev).bfloat16()
      out = torch.empty(nb, N, K, device=dev)
      if N % 128 == 0 and K % 384 == 0:
          s_big = big_splits(nb, R, N, K)
          big = timeit(lambda: gemm.wgrad_nt(dy, x, out, splits=s_big, big_tiles=True))
          print("   128x384 tiles %.1f us (%d splits, %.0f TFLOP/s incl. the slab sum)" % (big, s_big, 2.0 * nb * R * N * K / big * 1e-6))
      own = timeit(lambda: gemm.wgrad_nt(dy, x, out))
      was = gemm.OWN_WGRAD
      gemm.OWN_WGRAD = False
      lib_t = timeit(lambda: gemm.wgrad(dy, x, out))
      gemm.OWN_WGRAD = was
      fl = 2.0 * nb * R * N * K
      print("%-28s %10.1f %10.1f %8.2f   %d   (own %.0f TFLOP/s)" % (str((nb, R, N, K)), own, lib_t, lib_t / own,
            lib_.gm3d_gemm_nt_splits(nb, R, N, K), fl / own * 1e-6))

"""Where does a workgroup of the GELU-epilogue LDS-DMA GEMMs (csrc/gemm_dma.hip) spend its time?  A scratch copy of the kernel, built
into its own library (never into libgm3d_hip.so), reads wall_clock64() at five points of every workgroup -- entry, first K-stage
landed (behind the first barrier of the K-loop), end of the K-loop, tile staged in LDS (behind the barrier after the staging writes),
last global store issued -- keeps the four early values in registers and writes all five with ordinary vector stores at the end of
the kernel, so that no stamp sits between the counted waits.  The clock is the constant 100 MHz one (10 ns a tick).

    python tools/gelu_dma_probe.py [--src other/gemm_dma.hip] [--build-only]      (GPU box; the library is built once into tools/bin/)

Per case (M x 1536 x 384; fc1 + GELU with and without F, fc2-dX x GELU'; bm 64 / 128): the median and the 90th percentile over the
workgroups of each of the four spans, in microseconds, the whole workgroup, the launch seen by the stamps (last end - first entry)
and the launch timed by events.  --src probes another revision of the file, e.g. `git show REV:gm3d_amd/csrc/gemm_dma.hip > x.hip`
(profiles/gelu_dma_phases.txt: the kernel before and after its epilogue loads were hoisted); the tool stops if an anchor is missing."""
import argparse, ctypes, hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "gm3d_amd", "csrc")
BIN = os.path.join(ROOT, "tools", "bin")

# (anchor, replacement) alternatives per stamp: exactly one alternative of each group must match exactly once
PATCHES = [
    [("namespace gm3d {\n\nconstexpr int DBK", "namespace gm3d {\n__device__ unsigned long long* gm3d_probe_stamps = nullptr;\n\nconstexpr int DBK")],
    [("    if (logical >= total_tiles) return;\n", "    if (logical >= total_tiles) return;\n    const unsigned long long pt0 = wall_clock64();\n    unsigned long long pt1 = 0;\n")],
    [("        __builtin_amdgcn_s_barrier();                             // ... everybody's have, and nobody still reads the other buffer\n",
      "        __builtin_amdgcn_s_barrier();                             // ... everybody's have, and nobody still reads the other buffer\n"
      "        if (kt == 0) pt1 = wall_clock64();\n")],
    [("#undef GM3D_DMA_STAGE\n", "#undef GM3D_DMA_STAGE\n    const unsigned long long pt2 = wall_clock64();\n")],
    [("    __syncthreads();\n    if (EPI == 3) {\n", "    __syncthreads();\n    const unsigned long long pt3 = wall_clock64();\n    if (EPI == 3) {\n")],
    [("            colpart[(size_t)tile_m * N + n0 + tid] = s;\n        }\n    }\n}\n",
      "            colpart[(size_t)tile_m * N + n0 + tid] = s;\n        }\n    }\n"
      "    if (tid == 0 && gm3d_probe_stamps) {\n        unsigned long long* o = gm3d_probe_stamps + 8 * (size_t)blockIdx.x;\n"
      "        o[0] = pt0; o[1] = pt1; o[2] = pt2; o[3] = pt3; o[4] = wall_clock64();\n    }\n}\n")],
]
SETTER = ('\nextern "C" int gm3d_probe_set(void* p) {\n'
          "    return hipMemcpyToSymbol(HIP_SYMBOL(gm3d::gm3d_probe_stamps), &p, sizeof(p)) == hipSuccess ? 0 : 1;\n}\n")


def patched(src):
    t = open(src).read()
    for group in PATCHES:
        hits = [(a, b) for a, b in group if t.count(a) == 1]
        assert len(hits) == 1, "probe anchor not found exactly once in %s: %r" % (src, group[0][0][:70])
        t = t.replace(*hits[0])
    return t + SETTER


def library(src):
    text = patched(src)
    tag = hashlib.sha1(text.encode()).hexdigest()[:12]
    so = os.path.join(BIN, "gelu_dma_probe_%s.so" % tag)
    if not os.path.exists(so):
        os.makedirs(BIN, exist_ok=True)
        scratch = os.path.join(BIN, "gelu_dma_probe_%s.hip" % tag)
        open(scratch, "w").write(text)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-shared", "-I", CSRC,
                               "-I", os.path.join(ROOT, "include"), scratch, "-o", so])
    return so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(CSRC, "gemm_dma.hip"))
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    so = library(a.src)
    if a.build_only:
        print(so)
        return
    import torch
    lib = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    lib.gm3d_probe_set.argtypes = [vp]
    fwd, bwd = lib.gm3d_gemm_tn_bf16_dma_gelu, lib.gm3d_gemm_tn_bf16_dma_gelu_bwd
    fwd.argtypes = [vp] * 5 + [i32] * 8 + [vp]
    bwd.argtypes = [vp] * 6 + [i32] * 8 + [vp]
    K, N = 384, 1536
    print("# %s" % os.path.relpath(a.src, ROOT))
    print("# us, median / p90 over the workgroups: first = entry -> first K-stage landed, kloop = -> end of the K-loop, stage = -> tile staged,")
    print("# store = -> last global store issued, wg = the whole workgroup; launch = last end - first entry by the stamps, (events)")
    for M in (3200, 4096, 8192):
        x = torch.randn(M, K, device="cuda").bfloat16()
        w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
        b = torch.randn(N, device="cuda")
        f = torch.randn(M, N, device="cuda").bfloat16()
        g = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        cp = torch.empty((M + 63) // 64, N, device="cuda")
        big = torch.empty(64 << 20, device="cuda")               # 256 MB: a pass over it leaves f cold, as a forward pass does
        st = torch.cuda.current_stream().cuda_stream
        for bm in (64, 128):
            total = -(-M // bm) * (N // 192)
            grid = (total + 7) // 8 * 8
            for name in ("fc1+GELU", "fc1+GELU+F", "fc2dX*GELU'"):
                def launch():
                    if name.startswith("fc1"):
                        return fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), f.data_ptr() if name.endswith("F") else None, g.data_ptr(),
                                   M, N, K, K, K, N, N, bm, st)
                    return bwd(x.data_ptr(), w.data_ptr(), f.data_ptr(), b.data_ptr(), g.data_ptr(), cp.data_ptr(), M, N, K, K, K, N, N, bm, st)
                stamps = torch.zeros(grid * 8, dtype=torch.int64, device="cuda")
                assert lib.gm3d_probe_set(None) == 0
                for _ in range(3):
                    assert launch() == 0
                big.zero_()
                assert lib.gm3d_probe_set(stamps.data_ptr()) == 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                assert launch() == 0
                e1.record()
                torch.cuda.synchronize()
                assert lib.gm3d_probe_set(None) == 0
                s = stamps.view(grid, 8)[:, :5].cpu().double()
                s = s[s[:, 0] > 0]                                   # workgroups past the last tile return at once
                assert s.shape[0] == total and bool((s[:, 1:] >= s[:, :-1]).all())
                d = torch.cat([s[:, 1:] - s[:, :-1], (s[:, 4] - s[:, 0])[:, None]], 1) * 0.01
                cols = "  ".join("%s %5.2f /%5.2f" % (n, float(d[:, i].median()), float(d[:, i].quantile(0.9)))
                                 for i, n in enumerate(("first", "kloop", "stage", "store", "wg")))
                print("M=%4d bm=%3d %-12s wgs=%4d  %s  launch %5.1f (%5.1f)" % (M, bm, name, total, cols,
                      float(s[:, 4].max() - s[:, 0].min()) * 0.01, e0.elapsed_time(e1) * 1e3))


if __name__ == "__main__":
    main()

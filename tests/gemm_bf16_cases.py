"""The cases of the bf16 GEMM tests against fp64 (tests/test_gemm_bf16_cases_cpu.py, tests/test_gpu_gemm_bf16_fp64.py, and
tests/golden/make_gemm_bf16_bars.py, which writes the GELU terms of the bars): the cases, the input recipes, the fp64 reference, the
per-element bound and, for the CPU test, the restatement and the faults planted in it.  Nothing here imports the package under test;
the CPU test checks the lists below against gm3d_amd/gemm.py.

BOUND of a TN element, C = bf16(A . W^T + bias) with fp32 accumulation -- every term in fp64, from the same bf16 operands:

    ref   = x64 @ w64^T + b                 mag = |x64| @ |w64|^T + |b|
    acc   = gamma(K + 1) * mag              gamma(n) = n u / (1 - n u),  u = 2^-23
    bound = acc + 2^-8 * (|ref| + acc)

Products of bf16 numbers are exact in fp32, so `acc` is the standard bound of a length-K sum plus the bias add in ANY order; u is
2^-23 and not 2^-24 because the MFMA's internal summation is not documented as round-to-nearest per add (a faithful add has unit
roundoff 2^-23); 2^-8 is the half-ulp of the ONE bf16 rounding the kernels promise, taken of the fp32 value (at most |ref| + acc).
NT element (fp32 result, S row splits added in order): gamma(R + S) * mag.  The fp64 reference's own error, (K + 1) 2^-53 mag, is nine
orders below.  The restatement bf16(fp32 matmul + b) sits at 0.75 .. 0.99 of the bound on the graded inputs: it is tight.

INPUT FAMILIES, each from a CPU generator seeded from the case:

    graded   randn operands; row i of x times 2^((7 i mod 25) - 12), row j of w and bias[j] times 2^((11 j mod 25) - 12): the outputs
             of one product span 2^-24 .. 2^24, which a bar scaled by one global number cannot follow.  All magnitudes stay within
             2^+-40: no subnormals, no overflow
    cancel   graded with x[:, K/2:] = x[:, :K/2] and w[:, K/2:] = -w[:, :K/2]: the true product is exactly zero, the result is the
             bias; mag is large, ref is small
    exact    x in {-1, 0, 1}, every w row with at most EXACT_NNZ nonzeros, each +-1 (a column permutation where N == K <= 128), bias
             an integer in [-8, 8] or none: every partial sum and the result are integers of magnitude <= 256, exact in fp32 and in
             bf16 -- the kernel must match fp64 bit for bit whatever its summation order.  NT: dy and x in {-1, 0, 1}, the magnitude sum
             of an element is at most R <= 2^24

A TN case is (entry point of gemm.py, N, K, its own arguments); it is run at every M of TN_M (WS_M for the weight-stationary kernel:
one more length at which its persistent ring wraps) as row prefixes of ONE problem of M_MAX rows, with and without bias, on all three
families.  The ragged pairs of `linear_tn` are (K, N).

GELU terms (`m` of the issue: what the device erf costs, which cannot be derived).  Both are measured on the CPU by
tests/golden/make_gemm_bf16_bars.py as 3 x the distance of torch's fp32 GELU (GELU') from fp64 on the cases' own arguments, and
committed in tests/golden/gemm_bf16_bars.json; never from a kernel's output.  The graded arguments span 2^+-24, so the forward term is
kept per element: a GELU evaluated in fp32 as a/2 (1 + erf(a / sqrt 2)) is off by c 2^-24 |a| (the rounding of 1 + erf, times a/2),
and the table holds c: m = 3 c 2^-24 |a64|.  The backward term is absolute (GELU' is O(1)): mg = 3 x the largest distance."""
import collections
import json
import math
import os

import torch

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bf16_bars.json")

U = 2.0 ** -23
HALF_ULP = 2.0 ** -8
GELU_SLOPE = 1.13                   # max |GELU'| (1.1290 at 1.41)
FAMILIES = ("graded", "cancel", "exact")
EXACT_NNZ = 248                     # nonzeros of an `exact` w row: with |bias| <= 8 the magnitude sum stays <= 256
EXACT_BIAS = 8
TN_M = (1, 63, 65, 130)             # partial tiles on both tile heights (64, 128)
M_MAX = 130
WS_WRAP_M = 32 * 257 + 5            # more 32-row tiles than the persistent grid has workgroups: the ring wraps
WS_M = TN_M + (WS_WRAP_M,)
ROWS_ALONE = 33                     # rows [0, 33) computed alone == the same rows of the 130-row product

OWN_KT = (2, 4, 6, 8, 16, 18, 24)   # == gemm.OWN_KT (asserted by the CPU test)
OWN_K_LOOP = (192, 320)             # K / 64 outside OWN_KT: the run-time loop
OWN_RAGGED = ((8, 8), (40, 72), (96, 288), (288, 96), (72, 136))          # (K, N)
WS_NK = ((512, 256), (256, 512), (512, 384), (128, 256), (256, 128), (384, 512), (288, 96), (96, 96), (384, 96), (192, 96), (512, 96),
         (96, 384), (96, 288), (96, 192))          # every (N, K) gm3d_gemm_ws_supported admits (asserted by the CPU test)
WS_POOL_NK = ((256, 128), (384, 512), (96, 512))

Case = collections.namedtuple("Case", "kernel N K args")          # args: ((keyword, value), ...) of the entry point
NTCase = collections.namedtuple("NTCase", "nb R N K")


def gamma(n):
    return n * U / (1.0 - n * U)


def case_id(c):
    return "-".join([c.kernel, "N%d" % c.N, "K%d" % c.K] + ["%s%s" % kv for kv in c.args])


def nt_case_id(c):
    return "nb%d-R%d-N%d-K%d" % c


def tn_cases():
    out = [Case("linear_tn", 256, 64 * kt, ()) for kt in OWN_KT]
    out += [Case("linear_tn", 256, K, ()) for K in OWN_K_LOOP]
    out += [Case("linear_tn", N, K, ()) for K, N in OWN_RAGGED]
    for bm in (64, 128):
        out += [Case("linear_tn_ring", N, K, (("bm", bm),)) for K in (128, 384, 1536) for N in (128, 384)]
        out += [Case("linear_tn_ring", N, 128, (("bm", bm),)) for N in (8, 96, 136, 200)]
        out += [Case("linear_tn_ring96", N, 128, (("bm", bm),)) for N in (96, 192, 384)]
        out += [Case("linear_tn_dma", N, 384, (("bm", bm),)) for N in (192, 1152)]
        out += [Case("linear_tn_dmaw", 768, 128, (("bm", bm), ("bn", bn))) for bn in (128, 192, 256)]
    out += [Case("linear_tn_ws", N, K, ()) for N, K in WS_NK]
    return out


def fence_cases():
    """one graded case per TN kernel and tile form for the NaN fence (csrc/gemm.hip: its unrolled, run-time-loop and ragged forms)"""
    out = [Case("linear_tn", 256, 128, ()), Case("linear_tn", 256, 192, ()), Case("linear_tn", 72, 40, ()), Case("linear_tn", 96, 288, ())]
    for bm in (64, 128):
        out += [Case("linear_tn_ring", 384, 128, (("bm", bm),)), Case("linear_tn_ring", 200, 128, (("bm", bm),)),
                Case("linear_tn_ring96", 96, 128, (("bm", bm),)), Case("linear_tn_dma", 192, 384, (("bm", bm),))]
        out += [Case("linear_tn_dmaw", 768, 128, (("bm", bm), ("bn", bn))) for bn in (128, 192, 256)]
    out += [Case("linear_tn_ws", 512, 256, ()), Case("linear_tn_ws", 288, 96, ()), Case("linear_tn_ws", 96, 288, ())]
    return out


def rows_of(c):
    return WS_M if c.kernel == "linear_tn_ws" else TN_M


NT_NK = ((8, 8), (96, 96), (128, 384), (576, 192))
NT_R = (32, 96, 1024)               # the smallest R the contract admits (one 32-row stage); three stages (the contract admits no ragged
#                                     last stage: R % 32 == 0); the default row split is 2 slabs at 1024 rows (gm3d_gemm_nt_splits)
NT_MULTI = (NTCase(2, 96, 96, 96), NTCase(1, 1024, 128, 384), NTCase(3, 32, 576, 192))


def nt_cases():
    return [NTCase(2, R, N, K) for N, K in NT_NK for R in NT_R]


def nt_variants(c, default_splits):
    """the launches of one NT case -> [(name, splits, big_tiles, slab sum in the launch)]"""
    v = [("splits1", 1, False, False), ("default", None, False, False)]
    if c.R % 64 == 0:
        v.append(("splits2", 2, False, False))
        v.append(("sum2", 2, False, True))
        if default_splits > 2:
            v.append(("sum", None, False, True))
    if c.N % 128 == 0 and c.K % 384 == 0:
        v.append(("big1", 1, True, False))
        if c.R % 64 == 0:
            v.append(("big2", 2, True, False))
    return v


# fused epilogues: the kernels' own smallest (K, N); M = 65 and 130 rows (pool: groups * group_rows)
EPI_M = (65, 130)
GELU_CASES = (Case("linear_gelu", 128, 64, ()), Case("linear_gelu_dma", 192, 64, (("bm", 64),)), Case("linear_gelu_dma", 192, 64, (("bm", 128),)))
GELU_BWD_CASES = (Case("linear_gelu_bwd", 128, 64, ()), Case("linear_gelu_bwd_dma", 192, 64, (("bm", 64),)),
                  Case("linear_gelu_bwd_dma", 192, 64, (("bm", 128),)))
PoolCase = collections.namedtuple("PoolCase", "route N K group_rows args")       # route, args: what gemm.route_pool answers
POOL_GROUPS = {32: (3, 5), 16: (5, 9)}            # odd counts: the last tile of every kernel holds fewer groups than it has room for


def pool_cases():
    out = [PoolCase("own", 128, 64, 32, ()), PoolCase("dma", 128, 64, 32, (("bm", 128), ("bn", 128))),
           PoolCase("dma", 192, 64, 32, (("bm", 128), ("bn", 192)))]
    out += [PoolCase("ws", N, K, 32, ()) for N, K in WS_POOL_NK]
    out += [PoolCase("ws16", N, K, 16, (("group_rows", 16),)) for N, K in WS_POOL_NK]
    return out


def pool_case_id(c):
    return "-".join([c.route, "N%d" % c.N, "K%d" % c.K, "g%d" % c.group_rows] + ["%s%s" % kv for kv in c.args if kv[0] != "group_rows"])


# ---------------------------------------------------------------------------------------------------------------------------- inputs

def _grade(n, step):
    return torch.pow(2.0, ((step * torch.arange(n)) % 25 - 12).double()).float()


def _seed(tag, *ints):
    s = sum(ord(ch) * (i + 1) for i, ch in enumerate(tag))
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _ternary(shape, g):
    return torch.randint(-1, 2, shape, generator=g).float()


def tn_inputs(family, M, N, K, salt=0):
    """-> x (M,K) bf16, w (N,K) bf16, bias (N) f32 on the CPU (every value of x and w is a bf16 number by construction or rounding)"""
    g = torch.Generator().manual_seed(_seed(family, M, N, K, salt))
    if family == "exact":
        x = _ternary((M, K), g)
        w = torch.zeros(N, K)
        if N == K and K <= 128:
            w[torch.arange(N), torch.randperm(K, generator=g)] = 1.0
        else:
            nnz = min(K, EXACT_NNZ)
            idx = torch.rand(N, K, generator=g).argsort(dim=1)[:, :nnz]
            w.scatter_(1, idx, torch.randint(0, 2, (N, nnz), generator=g).float() * 2 - 1)
        b = torch.randint(-EXACT_BIAS, EXACT_BIAS + 1, (N,), generator=g).float()
        return x.bfloat16(), w.bfloat16(), b
    x = (torch.randn(M, K, generator=g) * _grade(M, 7)[:, None]).bfloat16()
    w = (torch.randn(N, K, generator=g) * _grade(N, 11)[:, None]).bfloat16()
    b = torch.randn(N, generator=g) * _grade(N, 11)
    if family == "cancel":
        h = K // 2
        x[:, h:2 * h] = x[:, :h]
        w[:, h:2 * h] = -w[:, :h]
    return x, w, b


def nt_inputs(family, c, salt=0):
    """-> dy (nb,R,N), x (nb,R,K) bf16 on the CPU.  graded: column j of dy times 2^((11 j mod 25) - 12), column k of x times
    2^((7 k mod 25) - 12) (the channels of a real weight gradient differ by orders of magnitude); cancel: the second half of the rows
    repeats the first in dy and negates it in x"""
    g = torch.Generator().manual_seed(_seed("nt" + family, c.nb, c.R, c.N, c.K, salt))
    if family == "exact":
        return _ternary((c.nb, c.R, c.N), g).bfloat16(), _ternary((c.nb, c.R, c.K), g).bfloat16()
    dy = (torch.randn(c.nb, c.R, c.N, generator=g) * _grade(c.N, 11)).bfloat16()
    x = (torch.randn(c.nb, c.R, c.K, generator=g) * _grade(c.K, 7)).bfloat16()
    if family == "cancel":
        h = c.R // 2
        dy[:, h:] = dy[:, :h]
        x[:, h:] = -x[:, :h]
    return dy, x


def gelu_bwd_inputs(M, N, K):
    """-> d_o (M,K), w2t (N,K) graded like x and w; f (M,N) bf16 = 3 randn and bias (N) = randn: GELU' arguments over its whole
    interesting range"""
    d_o, w2t, _ = tn_inputs("graded", M, N, K, salt=7)
    g = torch.Generator().manual_seed(_seed("gelubwd", M, N, K))
    return d_o, w2t, (torch.randn(M, N, generator=g) * 3.0).bfloat16(), torch.randn(N, generator=g)


# --------------------------------------------------------------------------------------------------- reference and bound (any device)

def tn_reference(x, w, b=None):
    """-> (ref, mag) in fp64"""
    x64, w64 = x.double(), w.double()
    ref, mag = x64 @ w64.t(), x64.abs() @ w64.abs().t()
    if b is not None:
        ref, mag = ref + b.double(), mag + b.double().abs()
    return ref, mag


def tn_bound(ref, mag, K):
    acc = gamma(K + 1) * mag
    return acc + HALF_ULP * (ref.abs() + acc)


def nt_reference(dy, x):
    d64, x64 = dy.double().transpose(-1, -2), x.double()
    return d64 @ x64, d64.abs() @ x64.abs()


def nt_bound(mag, R, splits):
    return gamma(R + splits) * mag


def gelu64(a):
    return 0.5 * a * (1.0 + torch.erf(a * math.sqrt(0.5)))


def gelu_grad64(a):
    return 0.5 * (1.0 + torch.erf(a * math.sqrt(0.5))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def gelu_bound(ref_f, bound_f, b, c_gelu):
    """G = bf16(GELU(bf16(F) + bias)) against g64 = gelu64(ref_F + b) -> (g64, bound): 1.13 * bound_F + 2^-8 |g64| + m, with
    m = 3 c 2^-24 |ref_F + b| (module docstring)"""
    a = ref_f + b.double()
    g = gelu64(a)
    return g, GELU_SLOPE * bound_f + HALF_ULP * g.abs() + 3.0 * c_gelu * 2.0 ** -24 * a.abs()


def gelu_bwd_bound(ref_dg, bound_dg, f, b, mg):
    """dF = bf16(fl32(bf16(dg) * gg)), gg = GELU'_fp32(fl32(f + b)) (the kernel's chain: the product rounded to bf16 like a stored GEMM
    result, one fp32 multiply, one bf16 rounding) against dg64 * GELU'64(f + b) -> (df64, pre, bound).  pre bounds the fp32 value
    the column sums add: (|gg64| + mg) bound_dg (the product's error through the factor) + mg |dg64| (the factor's error; mg also
    covers the fp32 rounding of f + b: |GELU''| <= 0.8) + 2^-23 |df64| (the multiply).  bound = pre + 2^-8 (|df64| + pre)."""
    gg = gelu_grad64(f.double() + b.double())
    df = ref_dg * gg
    pre = (gg.abs() + mg) * bound_dg + mg * ref_dg.abs() + U * df.abs()
    return df, pre, pre + HALF_ULP * (df.abs() + pre)


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 = 0, x / 0 = inf, NaN stays NaN) -> float"""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def locate(got, ref, bound):
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = tuple(int(v) for v in torch.unravel_index(r.argmax(), r.shape))
    return "element %s: %.9g against %.9g, bound %.3g" % (i, float(got[i]), float(ref[i]), float(bound[i]))


def bars():
    with open(TABLE) as f:
        return json.load(f)


# ----------------------------------------------------------------------------------- CPU: the restatement and the faults planted in it

def tn_restate(x, w, b=None):
    """what the kernels promise, on the CPU: an fp32 product, the bias added in fp32, ONE rounding to bf16"""
    y = x.float() @ w.float().t()
    return (y if b is None else y + b).bfloat16()


def nt_restate(dy, x):
    return dy.float().transpose(-1, -2) @ x.float()


FAULTS = ("drop_k8", "swap_rows", "zero_row", "move_small", "bias_late")
MOVE = 4e-3
BIAS_LATE_K = 384                   # beyond: not required (the margin shrinks as K grows)


def plant(fault, x, w, b):
    """-> the restatement with `fault` planted, or None where it does not apply.
    drop_k8: the last 8-chunk of K never multiplied; swap_rows: output rows 0 and 32 swapped; zero_row: the output row of the smallest
    x row zeroed; move_small: the element of the smallest magnitude sum among those with |ref| < 2^-8 moved by 4e-3; bias_late: the
    bias added after the bf16 rounding (two roundings)."""
    M, K = x.shape
    if fault == "drop_k8":
        return tn_restate(x[:, :K - 8], w[:, :K - 8], b) if K > 8 else None
    if fault == "bias_late":
        return None if b is None else (tn_restate(x, w).float() + b).bfloat16()
    y = tn_restate(x, w, b).clone()
    if fault == "swap_rows":
        if M <= 32:
            return None
        y[[0, 32]] = y[[32, 0]]
    elif fault == "zero_row":
        y[int(x.double().abs().sum(1).argmin())] = 0.0
    elif fault == "move_small":
        ref, mag = tn_reference(x, w, b)
        small = ref.abs() < HALF_ULP
        if not bool(small.any()):
            return None
        i = torch.unravel_index(torch.where(small, mag, torch.full_like(mag, float("inf"))).argmin(), mag.shape)
        y[i] = (y[i].float() + MOVE).bfloat16()
    return y

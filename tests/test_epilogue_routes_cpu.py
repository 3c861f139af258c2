"""No GPU: gemm.route_gelu / route_gelu_bwd / route_pool / route_bn, which launch nothing, must name what was launched.

For every fused-epilogue launch of tests/golden/epilogue_launches.json (recorded on the GPU before these functions existed), and for
every row pass that stands where one could have been, stand-in operands are rebuilt from the recorded M / N / K and pitches, the
matching route is asked under the case's switches, and its answer must be the entry point in the table with the same trailing
integers (bm, bn, group rows) and the same number of column-sum partial rows.  Every kind a route can answer is met at least once."""
import json

import pytest
import torch

from tests.golden import make_golden_epilogue_launches as E
from tests.golden.make_golden_gemm_routes import Fake

P = "gm3d_gemm_tn_bf16"
DT = {0: torch.float32, 1: torch.bfloat16}          # the C ABI's dtype ids
GELU = {P + "_dma_gelu": "dma", P + "_gelu": "own", "gm3d_bias_gelu_fwd": "split"}
GELU_BWD = {P + "_dma_gelu_bwd": "dma", P + "_gelu_bwd": "own", "gm3d_bias_gelu_bwd": "split"}
POOL = {P + "_dma_pool": "dma", P + "_pool": "own", "gm3d_group_max_fwd": "split"}      # and P_ws_pool: "ws" / "ws16" by its tail
BN = {P + "_ws_bn_stats": "stats", P + "_ws_bn_apply": "apply"}


@pytest.fixture(scope="module")
def table():
    with open(E.PATH) as f:
        return json.load(f)


def _pair(M, N, K, ldx=None, ldw=None, dtype=torch.bfloat16):
    """x (M,K), w (N,K) at the recorded pitches"""
    return Fake((M, K), dtype, (ldx or K, 1), 4096), Fake((N, K), dtype, (ldw or K, 1), 8192)


def _product_before(events, i):
    name, ints = events[i - 1]
    assert name.startswith(P), "a row pass stands behind the product it finishes, not behind %s" % name
    return ints[:5]


def test_stack_routes_name_what_the_stacks_launched(table):
    from gm3d_amd import gemm, masked_stack
    seen, seen_bwd = set(), set()
    for case, (family, _, sw) in E.CASES.items():
        if family not in ("stack", "masked"):
            continue
        events = table[case]
        with E.switches(sw):
            how = {"tiled": family == "stack", "fuse": family == "stack" or masked_stack.FUSE_GELU}
            for name, ints in events:
                if name in GELU:
                    if GELU[name] == "split":            # (R, C, dtype): the row pass behind fc1 = C/4 -> C
                        x, w = _pair(ints[0], ints[1], ints[1] // 4, dtype=DT[ints[2]])
                        tail = []
                    else:                                # M, N, K, pitches of x, w, f, g, then the kernel's own integers
                        x, w = _pair(*ints[:5])
                        tail = ints[7:]
                    kind, args = gemm.route_gelu(x, w, **how)
                    assert (kind, list(args.values())) == (GELU[name], tail), (case, name, ints, kind, args)
                    seen.add(kind)
                if name in GELU_BWD:
                    if GELU_BWD[name] == "split":
                        M, N, C, ldd, dtype, tail = ints[0], ints[1], ints[1] // 4, ints[1] // 4, DT[ints[2]], []
                    else:                                # M, N = hidden, K = C, pitches of d_o, w2t, f, df, then the kernel's own
                        M, N, C, ldd, dtype, tail = ints[0], ints[1], ints[2], ints[3], torch.bfloat16, ints[7:]
                    d_o, w2 = Fake((M, C), dtype, (ldd, 1), 4096), Fake((C, N), dtype, None, 8192)
                    kind, args, rows = gemm.route_gelu_bwd(d_o, w2, **how)
                    assert (kind, list(args.values())) == (GELU_BWD[name], tail), (case, name, ints, kind, args)
                    # the partials' second stage (J, rows * cols, rows, cols, ...) over the hidden width: the rows that were allocated
                    finish, = [e[1] for e in events if e[0] == "gm3d_colsum_finish_batched" and e[1][3] == N]
                    assert rows == finish[2], (case, name, rows, finish)
                    seen_bwd.add(kind)
    assert seen == seen_bwd == {"dma", "own", "split"}


def test_embed_routes_name_what_the_embed_launched(table):
    from gm3d_amd import gemm
    seen, seen_bn = set(), set()
    for case, (family, a, sw) in E.CASES.items():
        if family != "embed":
            continue
        events = table[case]
        k, train, selected = a["k"], a["train"], a["V"] is not None
        with E.switches(sw):
            for i, (name, ints) in enumerate(events):
                # ---- conv + max-pool: M, N, K, pitches of x and w, N, N, bias after the pool, then the kernel's own integers
                if name in POOL or name == P + "_ws_pool":
                    want = POOL.get(name) or ("ws16" if len(ints) == 9 else "ws")
                    x, w = _pair(*(_product_before(events, i) if want == "split" else ints[:5]))
                    kind, args = gemm.route_pool(x, w, k)
                    assert (kind, list(args.values())) == (want, [] if want == "split" else ints[8:]), (case, name, ints, kind, args)
                    seen.add(kind)
                # ---- conv3 + BatchNorm: M, N, K, pitches of x, w, t and the product, group rows; or the pass behind the plain product
                unfused = name == "gm3d_bn_bcast_stats" or (not train and name == "gm3d_bn_bcast_apply_relu")
                if name in BN or unfused:
                    M, N, K, ldx, ldw = _product_before(events, i) if unfused else ints[:5]
                    x, w = _pair(M, N, K, ldx, ldw)
                    t = Fake((M // k, N), torch.bfloat16, None, 16384)
                    kind, args = gemm.route_bn(x, w, t, k, train, selected)
                    assert (kind, list(args.values())) == (("none", []) if unfused else (BN[name], ints[7:])), (case, name, ints, kind, args)
                    seen_bn.add(kind)
    assert seen == {"ws16", "ws", "dma", "own", "split"} and seen_bn == {"stats", "apply", "none"}

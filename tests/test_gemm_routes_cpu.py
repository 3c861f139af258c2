"""No GPU: which entry point every dense product reaches, against the table committed before gemm.route / gemm.wgrad existed.

tests/golden/gemm_routes.json was written by tests/golden/make_golden_gemm_routes.py at the parent of the commit that introduced the
dispatcher (stand-in operands, `_launch` replaced by a recorder, the library calls recording themselves); the same generator run on
the code under test must reproduce it launch for launch, integer argument for integer argument.  And gemm.route, which launches
nothing, must name the target gemm.mm launched."""
import json
import os

import pytest
import torch

from tests.golden import make_golden_gemm_routes as G

_KIND = {"gm3d_gemm_tn_bf16": "own", "gm3d_gemm_tn_bf16_ring": "ring", "gm3d_gemm_tn_bf16_dmaw": "dmaw", "gm3d_gemm_tn_bf16_ws": "ws",
         "gm3d_gemm_tn_f32": "f32", "lib": "lib"}


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "gemm_routes.json")) as f:
        return json.load(f)


def test_every_product_reaches_the_entry_point_of_the_committed_table(table):
    got = json.loads(G.dumps(G.generate()))
    assert list(got) == list(table)
    wrong = [k for k in table if got[k] != table[k]]
    assert not wrong, (len(wrong), wrong[:5], got[wrong[0]], table[wrong[0]])


def test_route_names_the_target_mm_launches(table):
    from gm3d_amd import gemm
    seen = set()
    for M, N, K, layout, mode in G.mm_grid():
        x, w, _, out = G.operands(M, N, K, layout, torch.bfloat16 if mode == "bf16" else torch.float32)
        with G.recording(mode == "f32own"):
            kind, args = gemm.route(x, w, out)
        (name, _, ints), = table["mm %s %s %d %d %d" % (mode, layout, M, N, K)]
        assert kind == _KIND[name], (M, N, K, layout, mode, kind, name)
        if kind in ("own", "ring", "dmaw", "ws"):            # behind M, N, K and the three pitches: the kernel's own integers
            assert ints[6:] == list(args.values()), (M, N, K, layout, mode, args, ints)
        seen.add(kind)
    assert seen == set(_KIND.values())

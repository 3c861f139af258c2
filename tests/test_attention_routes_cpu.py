"""No GPU: attention.route / route_qkv, which launch nothing, must name what was launched.

tests/golden/attention_routes.json was recorded on the host before gm3d_amd/attention.py existed, through the wrappers the two block
stacks called then (tests/golden/make_golden_attention_routes.py).  The generator must reproduce it exactly from the code under test,
and for every row attention.route, asked with the caller's `head` / `pad`, must name the family (gm3d_attention_fwd/bwd: head,
_masked_: flash, _long_: stream) and the row count (the T among the launch's integers) of what ran.  All four answers -- the padded one
forward and backward -- are met."""
import json

import pytest
import torch

from tests.golden import make_golden_attention_routes as G
from tests.golden.make_golden_gemm_routes import Fake

FAMILY = {"gm3d_attention_fwd": ("head", False), "gm3d_attention_bwd": ("head", True),
          "gm3d_attention_masked_fwd": ("flash", False), "gm3d_attention_masked_bwd": ("flash", True),
          "gm3d_attention_long_fwd": ("stream", False), "gm3d_attention_long_bwd": ("stream", True)}


@pytest.fixture(scope="module")
def table():
    with open(G.PATH) as f:
        return f.read()


def test_the_generator_reproduces_the_committed_table(table):
    assert G.dumps(G.generate()) == table


def test_route_names_what_every_row_launched(table):
    from gm3d_amd import attention
    rows = json.loads(table)
    assert list(rows) == [G.key(*c) for c in G.grid()]
    seen = set()
    for c in G.grid():
        caller, dt, hd, masked, T = c
        events = rows[G.key(*c)]
        assert [FAMILY[e[0]][1] for e in events] == [False, True], (c, events)       # one forward, one backward
        head, pad = G.CALLERS[caller]
        for name, meta, ints in events:
            family, backward = FAMILY[name]
            got = attention.route(T, hd, G.DTYPES[dt], masked, backward, head=head, pad=pad)
            # the head launches carry (B, T, H, dtype), the others (B, T, H, hd, dtype)
            assert got == (family, ints[1]) and meta["T"] == ints[1], (c, name, ints, got)
            assert ("HD" in meta) == (family != "head")
            seen.add((got[0], "padded" if got[1] != T else "as is", backward))
            assert got[1] == T or (got[1] == attention.PAD_T and T < attention.PAD_T)
    assert seen == {(f, "as is", b) for f in ("head", "flash", "stream") for b in (False, True)} | {
        ("stream", "padded", False), ("stream", "padded", True)}


def test_route_qkv():
    """the qkv-fused launch: bf16, 33..64 tokens, dense 16-byte aligned operands, the caller's switch on"""
    from gm3d_amd import attention

    def ask(T, dtype=torch.bfloat16, fuse=True, base=4096):
        h, w = Fake((2 * T, 384), dtype, None, base), Fake((1152, 384), dtype, None, 8192)
        return bool(attention.route_qkv(h, w, T, 6, fuse))
    assert [ask(T) for T in (32, 33, 64, 65)] == [False, True, True, False]
    assert not ask(64, dtype=torch.float32)
    assert not ask(64, fuse=False)
    assert not ask(64, base=4096 + 8)
    assert ask(33) is True and ask(64, fuse=False) is False

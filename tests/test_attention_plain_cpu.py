"""CPU: the case list and the committed bars table of tests/test_gpu_attention_plain.py (tests/attention_plain_cases.py,
tests/golden/attention_plain_bars.json): one row per case, the table regenerates, every base row is at most half its bar, and the
cases reach every instantiation of the whole-head kernels, the three routes of an unmasked call and both dtypes."""
import importlib.util
import json
import os
import re

import pytest
import torch

from tests import attention_plain_cases as C
from tests import mattn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def committed():
    with open(C.TABLE) as f:
        return json.load(f)


def _routes(c):
    """(forward, backward | None) as attention.fwd / bwd route the case"""
    from gm3d_amd import attention
    dt, pad = R.DTYPES[c.dtype], c.call == "pad"
    f = attention.route(c.T, c.hd, dt, False, False, head=True, pad=pad)
    return f, (None if c.call == "fwd" else attention.route(c.T, c.hd, dt, False, True, head=True, pad=pad))


def test_table_has_exactly_one_row_per_case(committed):
    ids = [C.case_id(c) for c in C.cases()]
    assert len(set(ids)) == len(ids)
    assert sorted(committed) == sorted(ids)
    for c in C.cases():
        row = committed[C.case_id(c)]
        assert sorted(row) == C.metrics_of(c), C.case_id(c)
        assert all(0.0 <= v < float("inf") for v in row.values()), C.case_id(c)


def test_bar_rule(committed):
    """base: mattn_ref.BARS as they stand, the restatement within HALF of each (a base case that is not is a wrong case); amp and
    scale: max(bar, 3 x the restatement), and in bf16 the restatement's dQ / dK within AMP_BF16_MAX."""
    for c in C.cases():
        row = committed[C.case_id(c)]
        bar = C.bars(c, row)
        assert sorted(bar) == C.metrics_of(c)
        for k, v in row.items():
            if c.variant == "base":
                assert bar[k] == R.BARS[c.dtype][k]
                assert v <= 0.5 * bar[k], (C.case_id(c), k, v)
            else:
                assert bar[k] == max(R.BARS[c.dtype][k], 3.0 * v)
        if c.variant == "amp" and c.dtype == "bf16":
            assert max(row["dq"], row["dk"]) <= C.AMP_BF16_MAX, C.case_id(c)
    assert all(c.T >= 32 for c in C.cases() if c.variant == "amp")


def test_cases_are_what_the_kernels_branch_on():
    cs = C.cases()
    assert all(c.kind == "none" and c.T <= 512 for c in cs)
    assert {c.variant for c in cs} == set(C.VARIANTS) and {c.call for c in cs} == set(C.CALLS)
    assert {c.B for c in cs} == {3, 4, 43} and {c.hd for c in cs} == {16, 32, 64}
    for dt in R.DTYPES:
        head = [c for c in cs if c.dtype == dt and _routes(c)[0][0] == "head"]
        assert {c.T for c in head if c.variant == "base" and c.B == 4} == set(C.HEAD_T)
        assert {c.T for c in head if c.variant == "amp"} == set(C.HEAD_AMP_T)
        assert {c.T for c in head if c.variant == "scale"} == set(C.HEAD_SCALE_T)
        assert any(c.B == 43 and c.T == 64 for c in head) and any(c.B == 3 for c in head)
        assert 43 * C.H > 256                                              # more workgroups than the card has CUs
    assert all(C.scale_of(c) == c.hd ** -0.5 for c in cs if c.variant != "scale")
    m, e = torch.frexp(torch.tensor(C.SCALE))
    assert float(m) != 0.5                                                 # no power of two: s * scale rounds


def test_cases_reach_every_instantiation_of_the_whole_head_kernels():
    """gm3d_attention_fwd / _bwd pick a kernel by by_int<...>: bf16 by the tile count ceil(T / 32), fp32 by T <= 64.  Every listed value
    is reached, from both sides of each switch."""
    src = open(os.path.join(ROOT, "gm3d_amd", "csrc", "attention.hip")).read()
    for name in ("gm3d_attention_fwd", "gm3d_attention_bwd"):
        body = src[src.index('extern "C" int %s(' % name):]
        body = body[:body.index("\n}\n")]
        lists = [tuple(int(v) for v in m.split(",")) for m in re.findall(r"by_int<([0-9, ]+)>", body)]
        assert lists == [(1, 2, 3, 4), (2, 4)], name
        assert "by_int<1, 2, 3, 4>(nt," in body and "const int nt = (T + 31) / 32;" in body
        assert "by_int<2, 4>(T <= 64 ? 2 : 4," in body
    for dt in R.DTYPES:
        Ts = {c.T for c in C.cases() if c.dtype == dt and _routes(c) == (("head", c.T), ("head", c.T))}
        assert {(T + 31) // 32 for T in Ts} == {1, 2, 3, 4}
        assert {T <= 64 for T in Ts} == {True, False}
        for edge in (32, 64, 96):
            assert edge in Ts and edge + 1 in Ts
        assert 1 in Ts and 128 in Ts


def test_cases_reach_the_three_routes_of_an_unmasked_call_in_both_dtypes():
    from gm3d_amd import attention
    seen = {}
    for c in C.cases():
        f, b = _routes(c)
        seen.setdefault(c.dtype, set()).update({f[0] if f[1] == c.T else "padded", *([] if b is None else [b[0] if b[1] == c.T else "padded"])})
        if f[1] != c.T or (b is not None and b[1] != c.T):
            assert c.call == "pad" and attention.PAD_T == 513
    assert seen["f32"] == {"head", "flash"}                                # the padded form is bf16 only
    assert seen["bf16"] == {"head", "flash", "padded"}
    pad = {c.T: _routes(c) for c in C.cases() if c.call == "pad"}
    assert pad[257] == (("flash", 257), ("stream", 513))
    assert pad[480] == (("flash", 480), ("stream", 513))
    assert pad[481] == pad[512] == (("stream", 513), ("stream", 513))
    # what route can answer for an unmasked call of at most 512 tokens is one of these three, whatever the flags
    for T in (1, 128, 129, 256, 257, 480, 481, 512):
        for hd in (16, 32, 64):
            for dt in R.DTYPES.values():
                for backward in (False, True):
                    for head in (False, True):
                        for p in (False, True):
                            assert attention.route(T, hd, dt, False, backward, head, p) in (("head", T), ("flash", T), ("stream", 513))


def test_inputs_follow_the_recipe():
    c = C.Case("amp", "none", 33, 64, 4, "bf16", "full")
    qkv, dout, mask = C.inputs(c)
    assert qkv.dtype == dout.dtype == torch.bfloat16 and tuple(qkv.shape) == (4, 33, 3 * C.H * 64) and tuple(dout.shape) == (4, 33, C.H * 64)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (4, 33, 33) and not bool(mask.any())
    again = C.inputs(c)
    assert torch.equal(qkv, again[0]) and torch.equal(dout, again[1])
    base = C.inputs(c._replace(variant="base"))[0]
    assert not torch.equal(base, qkv)
    q, k, v = qkv.float().view(4, 33, 3, -1).unbind(2)
    assert 5.0 < float(q.std()) / float(v.std()) < 7.0 and 5.0 < float(k.std()) / float(v.std()) < 7.0
    s = torch.einsum("bthd,buhd->bhtu", q.view(4, 33, C.H, 64), k.view(4, 33, C.H, 64)) * C.scale_of(c)
    assert 150.0 < float(s.abs().max()) < 400.0                            # the logits `amp` is about


def test_locate_agrees_with_the_metrics():
    """the failure message's worst slice carries the error mattn_ref.errors reports"""
    for c in (C.Case("base", "none", 33, 64, 3, "f32", "full"), C.Case("base", "none", 1, 64, 4, "bf16", "full")):
        qkv, dout, mask = C.inputs(c)
        ref = C.reference(c, qkv, dout, mask)
        fn = R.emulate_bf16 if c.dtype == "bf16" else R.restate_f32
        got = list(fn(qkv, mask, C.H, c.hd, C.scale_of(c), dout))
        got[0] = got[0].clone()
        got[0].view(c.B, c.T, C.H, c.hd)[2, c.T // 2, 4, 7] += 0.5          # one element of cloud 2, head 4
        got[2] = got[2].clone()
        got[2].view(c.B, c.T, 3, C.H, c.hd)[1, 0, 1, 5, 3] += 0.25          # dK of cloud 1, head 5
        err = C.errors(c, got, ref, qkv, dout, mask)
        for k in C.metrics_of(c):
            e, where = C.locate(c, k, got, ref, qkv, dout)
            assert e == pytest.approx(err[k], rel=1e-12), (k, where)
        assert C.locate(c, "out", got, ref, qkv, dout)[1].startswith("cloud 2 head 4 row %d col 7:" % (c.T // 2))
        assert C.locate(c, "dk_zero" if c.T == 1 else "dk", got, ref, qkv, dout)[1].startswith("cloud 1 head 5 (row 0 col 3):")


def test_table_regenerates(committed):
    spec = importlib.util.spec_from_file_location("make_attention_plain_bars",
                                                  os.path.join(ROOT, "tests", "golden", "make_attention_plain_bars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.generate() == committed

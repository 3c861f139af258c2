"""No GPU: the two pure decisions behind every weight gradient, asked instead of launched.

gemm.route_wgrad on the stand-in operands of tests/golden/make_golden_gemm_routes.py must name the kind whose entry point
tests/golden/gemm_routes.json lists for the same case, with the same row splits (NT kernel) or row chunks and adding kernel
(library); gemm.multi_splits must give every combined launch of tests/golden/wgrad_launches.json (recorded on the GPU before
multi_splits existed) the splits it ran with."""
import json
import os

import torch

from tests.golden import make_golden_gemm_routes as G
from tests.golden import make_golden_wgrad_launches as W

_KIND = {"gm3d_gemm_nt_bf16": "nt", "gm3d_gemm_nt_f32": "f32", "lib": "lib"}


def test_route_wgrad_names_the_target_wgrad_launches():
    from gm3d_amd import gemm
    with open(os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "gemm_routes.json")) as f:
        table = json.load(f)
    keys = [k for k in table if k.startswith("wgrad ")]
    seen = set()
    for R, N, K, nb, mode in G.wgrad_grid():
        key = "wgrad %s %s %d %d %d" % (mode, "2d" if nb is None else "nb%d" % nb, R, N, K)
        dtype = torch.bfloat16 if mode == "bf16" else torch.float32
        lead = () if nb is None else (nb,)
        ops = [G.Fake(lead + (R, N), dtype, None, 4096), G.Fake(lead + (R, K), dtype, None, 8192)]
        if nb is not None:
            ops.append(G.Fake((nb, N, K), torch.float32, None, 16384))
        with G.recording(mode == "f32own"):
            kind, args = gemm.route_wgrad(*ops)
        events = table[key]
        name, _, ints = events[0]
        assert kind == _KIND[name], (key, kind, name)
        if kind == "nt":
            assert args == {"splits": ints[10]}, (key, args, ints)
            assert (len(events) == 2) == (args["splits"] > 1)
        elif kind == "lib":
            assert args == {"S": ints[0] // (nb or 1), "adder": events[1][0] if len(events) > 1 else None}, (key, args, events)
        seen.add(kind)
        keys.remove(key)
    assert not keys and seen == {"nt", "f32", "lib"}       # ("pad" needs the ragged widths off: tests/test_gpu_routing.py)


def test_pad_route_is_the_nt_kernel_on_one_zero_padded_tile(monkeypatch):
    """ragged widths off: a narrow bf16 layer takes "pad" exactly where the NT kernel takes a (1, R, 128) copy of dy beside x"""
    from gm3d_amd import gemm
    monkeypatch.setattr(gemm, "RAGGED", False)
    kinds = {}
    for R in G.WG_RS:
        for N, K in ((96, 384), (96, 128), (8, 72), (128, 128)):
            dy, x = G.Fake((R, N), torch.bfloat16, None, 4096), G.Fake((R, K), torch.bfloat16, None, 8192)
            kind, args = gemm.route_wgrad(dy, x)
            padded = N < 128 and gemm.wgrad_supported(G.Fake((1, R, 128), torch.bfloat16), x.unsqueeze(0))
            assert (kind == "pad") == padded, (R, N, K, kind)
            if padded:
                assert args == {"splits": gemm.lib.gm3d_gemm_nt_splits(1, R, 128, K)}
            kinds[kind] = kinds.get(kind, 0) + 1
    assert set(kinds) == {"pad", "nt", "lib"}, kinds


def _multi_launches():
    with open(W.PATH) as f:
        table = json.load(f)
    found = [(case, ev[3]) for case, events in table.items() for ev in events if ev[0] == "gm3d_gemm_nt_bf16_multi"]
    assert len(found) >= 10 and any(len(m["problems"]) > 8 for _, m in found)
    return found


def test_multi_splits_gives_every_recorded_launch_its_splits():
    from gm3d_amd import gemm
    for case, meta in _multi_launches():
        assert gemm.multi_splits([tuple(p) for p in meta["problems"]]) == meta["splits"], (case, meta)


def test_multi_splits_returns_explicit_splits_unchanged():
    from gm3d_amd import gemm
    for case, meta in _multi_launches():
        given = [3 + i for i in range(len(meta["problems"]))]
        assert gemm.multi_splits([tuple(p) for p in meta["problems"]], splits=given) == given, case


def _recorded_many(monkeypatch, n, bad=()):
    """wgrads._many over n stand-in requests (request i fails wgrad_multi_ok when i is in `bad`) -> (calls, results): the launchers
    are recorders that return their requests' numbers"""
    from gm3d_amd import gemm, wgrads
    calls = []
    monkeypatch.setattr(gemm, "wgrad_multi_ok", lambda dy, x, out: dy not in bad)
    monkeypatch.setattr(gemm, "wgrad_nt_multi", lambda reqs: calls.append(("multi", [r[0] for r in reqs])) or [r[0] for r in reqs])
    monkeypatch.setattr(gemm, "wgrad", lambda dy, x, out=None: calls.append(("one", dy)) or dy)
    return calls, wgrads._many([(i, "x%d" % i, "out%d" % i) for i in range(n)])


def test_many_cuts_more_than_16_requests_into_equal_launches_in_order(monkeypatch):
    """ceil(n / 16) launches of ceil(n / ceil(n / 16)) requests each, in arrival order; a chunk of one goes through gemm.wgrad; the
    results come back in the order of the requests.  (No step of the models defers more than 15: wgrad_launches.json cannot pin this.)"""
    for n, sizes in ((2, [2]), (15, [15]), (16, [16]), (17, [9, 8]), (32, [16, 16]), (33, [11, 11, 11]), (49, [13, 13, 13, 10]),
                     (241, [16] * 15 + [1])):
        assert -(-n // 16) == len(sizes) and max(sizes) == -(-n // len(sizes)) and sum(sizes) == n
        calls, res = _recorded_many(monkeypatch, n)
        assert res == list(range(n)), n
        assert [len(c[1]) if c[0] == "multi" else 1 for c in calls] == sizes, (n, calls)
        assert [c[0] for c in calls] == ["multi" if s > 1 else "one" for s in sizes]
        flat = [i for c in calls for i in (c[1] if c[0] == "multi" else [c[1]])]
        assert flat == list(range(n)), n


def test_many_sends_all_to_wgrad_when_one_request_fails_or_the_switch_is_off(monkeypatch):
    from gm3d_amd import gemm
    for n, bad in ((1, ()), (4, (2,)), (20, (19,))):
        calls, res = _recorded_many(monkeypatch, n, bad)
        assert calls == [("one", i) for i in range(n)] and res == list(range(n))
    monkeypatch.setattr(gemm, "MULTI_WGRAD", False)
    calls, res = _recorded_many(monkeypatch, 20)
    assert calls == [("one", i) for i in range(20)] and res == list(range(20))

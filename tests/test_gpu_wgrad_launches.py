"""-m gpu: the weight-gradient launches of the training steps and of the mini-PointNet embed, against the table recorded before
gm3d_amd/wgrads.py scheduled them.

tests/golden/wgrad_launches.json was written by tests/golden/make_golden_wgrad_launches.py on the GPU at the parent of the commit that
moved the scheduling (fork, defer, combine, the embed's batch) into wgrads.py and the decisions into gemm.route_wgrad /
gemm.multi_splits.  The same generator, run on the code under test, must reproduce it launch for launch: name, integer arguments,
main or side stream, the problems and row splits of every combined launch, the region stream's fork and join, in the same host order;
a case on one side only is a failure.  No step defers more than 15 requests, so the chunks beyond 16 are asked directly below."""
import json

import pytest

from tests.golden import make_golden_wgrad_launches as W

pytestmark = pytest.mark.gpu


def test_every_case_launches_what_the_committed_table_lists():
    with open(W.PATH) as f:
        want = json.load(f)
    got = json.loads(W.dumps(W.generate()))
    assert list(want) == list(W.CASES), "the table and the generator's cases differ"
    assert list(got) == list(want)
    for k in want:
        first = next((i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b), min(len(got[k]), len(want[k])))
        assert got[k] == want[k], "%s: launch %d is %s, the table has %s (%d launches against %d)" % (
            k, first, got[k][first:first + 1], want[k][first:first + 1], len(got[k]), len(want[k]))


def _req(i, R, N, K):
    import torch
    g = torch.Generator().manual_seed(100 + i)
    return (torch.randn(1, R, N, generator=g).cuda().bfloat16(), torch.randn(1, R, K, generator=g).cuda().bfloat16(), None)


def test_seventeen_requests_run_as_two_launches_with_the_bits_of_the_single_kernel():
    """No step of the models defers more than 15 requests, so the chunking beyond 16 is asked directly: 17 requests through
    wgrads._many are two combined launches of 9 and 8 in arrival order, and every result has the bits of wgrad_nt on that request alone
    with the splits gemm.multi_splits gives it inside its chunk."""
    import torch
    from gm3d_amd import gemm, wgrads
    shapes = [(64, 128, 128), (8192, 96, 384), (256, 384, 96), (4096, 128, 256), (32, 8, 72), (1024, 192, 192)]
    reqs = [_req(i, *shapes[i % len(shapes)]) for i in range(17)]
    reqs[3] = reqs[3][:2] + (torch.full((1, 128, 256), float("nan"), device="cuda"),)        # a destination given by the caller
    del W._events[:]
    with W.recording():
        res = wgrads._many(reqs)
        torch.cuda.synchronize()
    multi = [e for e in W._events if e[0] == "gm3d_gemm_nt_bf16_multi"]
    problems = [[1, dy.shape[1], dy.shape[2], x.shape[2]] for dy, x, _ in reqs]
    assert [m[3]["problems"] for m in multi] == [problems[:9], problems[9:]]
    assert [e[0] for e in W._events if e[0].startswith("gm3d_gemm_nt")] == ["gm3d_gemm_nt_bf16_multi"] * 2
    assert len(res) == 17 and res[3] is reqs[3][2]
    want_splits = gemm.multi_splits([tuple(p) for p in problems[:9]]) + gemm.multi_splits([tuple(p) for p in problems[9:]])
    assert [s for m in multi for s in m[3]["splits"]] == want_splits and max(want_splits) > 1
    for (dy, x, _), got, s in zip(reqs, res, want_splits):
        assert torch.equal(got, gemm.wgrad_nt(dy, x, splits=s)), (tuple(dy.shape), tuple(x.shape), s)


def test_a_batch_of_one_request_runs_alone_on_its_own_default_splits():
    """wgrads.Batch with exactly one request the NT kernel takes (the others, 48 rows, run at once): flush launches gm3d_gemm_nt_bf16
    with gm3d_gemm_nt_splits of that request alone, not the combined launch."""
    import torch
    from gm3d_amd import gemm, wgrads
    dy, x, _ = _req(0, 8192, 96, 384)
    small = [_req(1 + i, 48, 96, 384) for i in range(2)]
    del W._events[:]
    with W.recording():
        batch = wgrads.Batch(torch.bfloat16)
        now = [batch.add(a[0], b[0]) for a, b, _ in small[:1]]
        later = batch.add(dy[0], x[0])
        now += [batch.add(a[0], b[0]) for a, b, _ in small[1:]]
        assert len(batch.reqs) == 1
        batch.flush()
        torch.cuda.synchronize()
    own = gemm.lib.gm3d_gemm_nt_splits(1, 8192, 96, 384)
    assert own > 1
    nt = [e for e in W._events if e[0].startswith("gm3d_gemm_nt")]
    assert [e[0] for e in nt] == ["gm3d_gemm_nt_bf16"] and nt[0][1][:4] == [1, 8192, 96, 384] and nt[0][1][10] == own
    assert torch.equal(later, gemm.wgrad_nt(dy, x)[0])
    for (a, b, _), got in zip(small, now):
        assert torch.equal(got, gemm.wgrad(a[0], b[0]))

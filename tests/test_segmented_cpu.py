"""CPU: segmented.SegmentedStep itself -- the part of the data-parallel pretrain step that both models share -- through a minimal
subclass whose segments are stubs: where _store puts a segment's gradients, the order in which _run issues phases, collectives
and waits (with and without gradient accumulation), and _reduce / _wait through a real gloo group of two ranks."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gm3d_amd.segmented import SegmentedStep


class _Opt:
    """What SegmentedStep reads of FlatAdamWEma: the flat gradient buffer, its per-parameter views, the segment layout."""

    def __init__(self, sizes_by_segment):
        sizes = [n for ns in sizes_by_segment for n in ns]
        self.G = torch.zeros(sum(sizes))
        self.gviews, self.segment_params, self.segment_ranges, off = [], {}, {}, 0
        for sg, ns in enumerate(sizes_by_segment):
            lo = off
            for n in ns:
                self.gviews.append(self.G[off:off + n])
                off += n
            self.segment_ranges[sg] = (lo, off)
        self._params = [torch.nn.Parameter(torch.zeros(v.numel())) for v in self.gviews]
        it = iter(self._params)
        for sg, ns in enumerate(sizes_by_segment):
            self.segment_params[sg] = [next(it) for _ in ns]
        self.accumulated = []

    def flat_grad_views(self):
        return list(zip(self._params, self.gviews))

    def accumulate(self, last):
        self.accumulated.append(last)


def _step(nseg, opt, accum=1, log=None):
    class Stub(SegmentedStep):
        NSEG = nseg

        def _segment(self, k, first_input=None):
            log.append("p%d" % k)

        def _reduce(self, seg):
            log.append("r%d" % seg)
            return (SimpleNamespace(wait=lambda: log.append("w%d" % seg)), None)

    return Stub(torch.nn.Identity(), None, opt, SimpleNamespace(accum_iter=accum), 0, broadcast=False)


def test_store_skips_aliased_copies_present_and_zeroes_missing(monkeypatch):
    opt = _Opt([(3, 4, 5)])
    step = _step(1, opt)
    opt.G.copy_(torch.arange(1.0, 13.0))
    v0, v1, v2 = step.seg_views[0]
    assert [v.numel() for v in (v0, v1, v2)] == [3, 4, 5] and v0.data_ptr() == opt.G.data_ptr()
    g2 = torch.arange(5.0) - 20.0
    copies, zeros = [], []
    real_copy, real_zero = torch._foreach_copy_, torch._foreach_zero_
    monkeypatch.setattr(torch, "_foreach_copy_", lambda dst, src: (copies.append([d.data_ptr() for d in dst]), real_copy(dst, src))[1])
    monkeypatch.setattr(torch, "_foreach_zero_", lambda dst: (zeros.append([d.data_ptr() for d in dst]), real_zero(dst))[1])
    step._store(0, (v0, None, g2))
    assert torch.equal(v0, torch.tensor([1.0, 2.0, 3.0]))              # already in its slot: untouched
    assert torch.equal(v1, torch.zeros(4))                             # no gradient: zeros
    assert torch.equal(v2, g2) and v2.data_ptr() != g2.data_ptr()      # copied into the flat buffer
    assert copies == [[v2.data_ptr()]] and zeros == [[v1.data_ptr()]]  # one multi-tensor call each, none on the aliased slot


@pytest.mark.parametrize("nseg", [3, 4])
def test_run_issues_each_collective_right_behind_its_phase(nseg):
    log = []
    step = _step(nseg, _Opt([(2,)] * nseg), log=log)
    phases = [lambda k=k: step._segment(k) for k in range(nseg)]
    assert step._run(phases) is True
    expect = [s % k for k in range(nseg) for s in ("p%d", "r%d")] + ["w%d" % k for k in range(nseg)]
    assert log == expect
    assert step.opt.accumulated == []


def test_run_with_accumulation_reduces_once_per_window():
    log, nseg = [], 3
    opt = _Opt([(2,)] * nseg)
    step = _step(nseg, opt, accum=3, log=log)
    phases = [lambda k=k: step._segment(k) for k in range(nseg)]
    got = []
    for update in (False, False, True):
        got.append(step._run(phases, update))
        if not update:
            assert not [e for e in log if e[0] in "rw"]
    assert got == [False, False, True]
    assert opt.accumulated == [False, False, True]
    assert log == ["p0", "p1", "p2"] * 3 + ["r0", "r1", "r2", "w0", "w1", "w2"]


class _Noop(SegmentedStep):
    NSEG = 2

    def _segment(self, k, first_input=None):
        pass


def test_reduce_without_a_process_group_is_none_and_wait_accepts_it():
    assert not dist.is_initialized()
    opt = _Opt([(6,), (10,)])
    step = _Noop(torch.nn.Identity(), None, opt, SimpleNamespace(), 0, broadcast=False)
    assert step.world == 1 and not step._avg and step.accum == 1
    opt.G.fill_(3.0)
    assert step._reduce(0) is None and step._reduce(1) is None
    step._wait([None, None])
    assert step._run([lambda: None] * 2) is True and opt.G.eq(3.0).all()


def _gloo_rank(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    opt = _Opt([(6,), (10,)])
    step = _Noop(torch.nn.Identity(), None, opt, SimpleNamespace(accum_iter=1), 0, broadcast=False)
    opt.G.fill_(float(rank + 1))
    done = step._run([lambda: None] * 2)
    q.put((rank, done, step.world, bool(step._avg), opt.G.numpy().copy()))      # numpy: no shm handles
    dist.barrier()
    dist.destroy_process_group()


def test_reduce_and_wait_average_over_two_gloo_ranks():
    """gloo has no ReduceOp.AVG: the SUM + div_(world) path."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, done, world, avg, G in res:
        assert done is True and world == 2 and avg is False
        assert G.shape == (16,) and (G == 1.5).all(), (rank, G)

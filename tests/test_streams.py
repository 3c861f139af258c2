"""gm3d_amd/streams.py: the audit that turns an unjoined side stream inside a hipGraph capture into a Python error
(the record is gpurun_out/segv.txt: SIGSEGV inside capture_end).  Ledger logic on the CPU with stand-in streams;
one GPU test that the real capture of the pretrain step raises -- and that the process survives.
What feeds the captured steps (SideStage, PinnedFeed, LookAhead) on toy producers: the ordering the overlapped engines depend on."""
from types import SimpleNamespace

import pytest
import torch

from gm3d_amd import streams as S


class FakeStream:
    n = 0

    def __init__(self):
        FakeStream.n += 1
        self.cuda_stream = FakeStream.n
        self.waited = []

    def wait_stream(self, other):
        self.waited.append(other.cuda_stream)


@pytest.fixture
def ledger():
    origin = FakeStream()
    led = S._Ledger(origin)
    S._ledgers.append(led)
    yield origin, led
    S._ledgers.pop()


def test_fork_join_closes(ledger):
    origin, led = ledger
    a = FakeStream()
    S.fork(a, origin, who="A")
    assert [w for _, w in S.open_streams()] == ["A"]
    S.join(a, origin)
    assert S.open_streams() == [] and origin.waited == [a.cuda_stream] and a.waited == [origin.cuda_stream]


def test_nested_fork_joined_into_its_parent_reopens_the_parent(ledger):
    origin, led = ledger
    a, b = FakeStream(), FakeStream()
    S.fork(a, origin, who="A")
    S.fork(b, a, who="B")           # forked while running on A
    S.join(a, origin)               # A comes back first ...
    S.join(b, a)                    # ... then B is joined into A, which the origin no longer waits for
    left = S.open_streams()
    assert len(left) == 1 and left[0][0] is a and "B" in left[0][1]
    S.join(a, origin)
    assert S.open_streams() == []


def test_nested_fork_joined_straight_into_the_origin(ledger):
    origin, led = ledger
    a, b = FakeStream(), FakeStream()
    S.fork(a, origin, who="A")
    S.fork(b, a, who="B")
    S.join(b, origin)
    S.join(a, origin)
    assert S.open_streams() == []


def test_forking_the_origin_itself_is_not_booked(ledger):
    origin, led = ledger
    other = FakeStream()
    S.fork(origin, other, who="origin waits for a producer")
    assert S.open_streams() == []


def test_outside_a_capture_nothing_is_booked():
    a, b = FakeStream(), FakeStream()
    S.fork(a, b, who="x")
    assert S.open_streams() == [] and a.waited == [b.cuda_stream]


def test_look_ahead_moves_fine_tune_items_one_ahead():
    """Items shaped like the fine-tune loader's (taxonomy, model_id, (points, label)); the mover picks what goes to the device."""
    items = [("tax%d" % i, "id%d" % i, (torch.full((2, 4, 3), float(i)), torch.tensor([i, i]))) for i in range(3)]
    moved = []

    def move(item):
        moved.append(item[0])
        return item[2][0].clone(), item[2][1].clone()

    la = S.LookAhead(items, move)
    assert len(la) == 3 and la.next is None
    seen = []
    for points, label in la:
        seen.append((float(points[0, 0, 0]), int(label[0]), None if la.next is None else float(la.next[0][0, 0, 0]), len(moved)))
    # item i + 1 has been moved when item i is handed out, and nothing is moved twice
    assert seen == [(0.0, 0, 1.0, 2), (1.0, 1, 2.0, 3), (2.0, 2, None, 3)] and la.next is None
    assert moved == ["tax0", "tax1", "tax2"]
    empty = S.LookAhead([], move)
    assert len(empty) == 0 and list(empty) == [] and empty.next is None and len(moved) == 3


def _staged_calls(batches, look_ahead, generator=None):
    """A toy overlapped step over `batches`: the producer graph on a SideStage, the caller's copy-out, a consumer graph on the current
    stream.  look_ahead(i): is batch i + 1 handed to call i?  -> every call's output (clones); ONE synchronisation, at the end."""
    static_in = torch.zeros_like(batches[0])
    stage = S.SideStage(static_in.device)
    if generator is None:
        staged = stage.capture(lambda: static_in * 2 + 1)
    else:
        staged = stage.capture(lambda: static_in + torch.rand(static_in.shape, device=static_in.device, generator=generator),
                               generator=generator)
    train_in = torch.zeros_like(staged)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with S.capture(graph):
        out = train_in * 3 - 1
    outs = []
    for i, b in enumerate(batches):
        stage.take(b, static_in)
        train_in.copy_(staged)
        if i + 1 < len(batches) and look_ahead(i):
            stage.enqueue(batches[i + 1], static_in)
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    return outs


_LOOK_AHEAD = {"always": lambda i: True, "never": lambda i: False, "alternately": lambda i: i % 2 == 0}


@pytest.mark.gpu
@pytest.mark.parametrize("how", sorted(_LOOK_AHEAD))
def test_side_stage_hands_every_call_its_own_batch(how):
    """Small integers: (b * 2 + 1) * 3 - 1 is exact in fp32, so every call's output equals the directly computed value."""
    batches = [torch.arange(48, dtype=torch.float32, device="cuda").reshape(2, 8, 3) + 100 * i for i in range(6)]
    outs = _staged_calls(batches, _LOOK_AHEAD[how])
    assert len(outs) == 6
    for b, o in zip(batches, outs):
        assert torch.equal(o, (b * 2 + 1) * 3 - 1)


@pytest.mark.gpu
def test_side_stage_generator_draws_do_not_depend_on_look_ahead():
    """The producer graph draws from a generator registered with it alone: same sequence of draws whatever the replay order."""
    batches = [torch.full((2, 8, 3), float(i), device="cuda") for i in range(6)]
    runs = {}
    for how, fn in _LOOK_AHEAD.items():
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        runs[how] = _staged_calls(batches, fn, generator=g)
    for how in ("never", "alternately"):
        assert all(torch.equal(a, b) for a, b in zip(runs["always"], runs[how])), how
    draws = [(o + 1) / 3 - b for o, b in zip(runs["always"], batches)]          # approximately: enough to tell two draws apart
    assert all(not torch.allclose(draws[0], d, atol=1e-3) for d in draws[1:])


@pytest.mark.gpu
def test_pinned_feed_delivers_every_push_while_the_stream_lags():
    """Six pushes through two pinned images behind ~10 ms of queued products: from the third push on an image is reused, and must
    not be overwritten before the copy that reads it has run."""
    import numpy as np
    a = torch.zeros(5, 7, dtype=torch.long, device="cuda")
    b = torch.zeros(3, 4, 3, dtype=torch.float32, device="cuda")
    feed = S.PinnedFeed(a, b)
    rng = np.random.RandomState(0)
    arrays = [(rng.randint(0, 1000, (5, 7)).astype(np.int64), rng.rand(3, 4, 3).astype(np.float32)) for _ in range(6)]
    big = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    for _ in range(8):
        big = big @ big * 1e-4
    clones = []
    for arr in arrays:
        feed.push(arr)
        clones.append((a.clone(), b.clone()))
    torch.cuda.synchronize()
    for (ca, cb), (xa, xb) in zip(clones, arrays):
        assert torch.equal(ca.cpu(), torch.from_numpy(xa)) and torch.equal(cb.cpu(), torch.from_numpy(xb))


@pytest.mark.gpu
def test_unjoined_side_stream_in_the_step_capture_raises_and_the_process_lives():
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    from tests import clouds
    B = 4
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
    torch.manual_seed(0)
    m = M.mae_vit_base_patch16_dec512d8b().cuda().train()
    ema = E.ModelEma(m, 0.999)
    opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema)
    x = clouds.uniform(B, 1024, 5).cuda()
    rogue = torch.cuda.Stream()
    scratch = torch.zeros(1024, device="cuda")

    def leaky(model, model_ema, samples, epoch, a, **kw):
        out = E.step_forward_backward(model, model_ema, samples, epoch, a, **kw)
        if torch.cuda.is_current_stream_capturing():
            S.fork(rogue, who="test: rogue fork that nobody joins")
            with torch.cuda.stream(rogue):
                scratch.add_(1.0)
        return out

    with pytest.raises(RuntimeError, match="rogue fork that nobody joins"):
        E.GraphedPretrainStep(m, ema, opt, args, x, 200, fwd_bwd=leaky)
    torch.cuda.synchronize()
    # the audit joined the stream before the capture ended: the runtime is intact and the same model captures cleanly
    g = E.GraphedPretrainStep(m, ema, opt, args, x, 200)
    o = g(x)
    torch.cuda.synchronize()
    assert float(o["loss"]) == float(o["loss"])
    assert S.open_streams() == []


@pytest.mark.gpu
def test_a_cached_weight_cast_is_waited_for_across_streams():
    """fused.weight_cache.get casts a weight once and hands the copy to whoever asks next.  The parallel inference chains of run_stack ask
    from DIFFERENT streams a few microseconds apart: the second one must wait for the casting launch (round 4: the teacher's forward as
    two chains differed from the single chain once in a full test run beside a loader process -- eager mode with un-pinned weights)."""
    import torch
    from gm3d_amd import fused
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    w = torch.randn(2048, 2048, device="cuda")
    big = torch.randn(8192, 8192, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        for _ in range(20):                       # keeps stream a busy: the cast below is queued behind ~100 ms of products
            big = big @ big * 1e-4
        c1 = fused.weight_cache.get(w, torch.bfloat16)
    with torch.cuda.stream(b):                    # no dependency on stream a except through the cache
        c2 = fused.weight_cache.get(w, torch.bfloat16)
        got = c2.float().abs().sum()
    torch.cuda.synchronize()
    assert c2 is c1
    assert float(got) == float(w.bfloat16().float().abs().sum())

"""Side streams inside hipGraph captures: every fork is booked, every capture is audited before it ends.

Why this exists (gpurun_out/segv.txt of round 3): a stream that joined a capture (it waited on an event of the
capturing stream) and is not waited on again by the capture-origin stream before `hipStreamEndCapture` is an "unjoined"
capture.  The runtime is specified to return an error for it; on this stack it took the process down with SIGSEGV inside
`torch.cuda.graphs.capture_end` -- no Python error, the test run simply died.  The product forks side streams in four places
(the decoders' second branch, the EMA teacher's parallel chains, the weight-gradient stream of a backward region, the data-
parallel step's warm-up), some of them nested (a stack node running ON the decoders' side stream forks the weight-gradient
stream), and switches (`wgrads.ASYNC_WGRAD`, `NOGRAD_SPLIT`, `GM3D_PARALLEL_DECODERS`) recombine them.

    fork(side, who=...)      side waits for the current stream; booked as open while a capture is being audited
    join(side)               the current stream waits for side; booked as closed.  Joining INTO a stream that is itself a
                             fork re-opens that stream (it now carries the joined work and must reach the origin too)
    with capture(graph): ..  torch.cuda.graph + the audit: at the end of the body every booked stream must be closed.
                             An open one is joined to the origin by the audit itself (so that ending the capture is safe)
                             and then reported as RuntimeError naming who forked it.

Outside a capture fork / join are plain wait_stream calls.
SideStage, PinnedFeed, LookAhead: what feeds the captured steps between replays (a producer graph on a second stream one batch
ahead, host draws through pinned memory, the loader one item ahead)."""
import contextlib
import sys

import torch
import torch.distributed as dist

_ledgers = []          # stack of active audits (captures do not nest in the product; the stack keeps the code honest if they do)


class _Ledger:
    def __init__(self, origin):
        self.origin = origin
        self.open = {}             # cuda_stream handle -> (stream, who forked it / why it is open)

    def is_origin(self, s):
        return s.cuda_stream == self.origin.cuda_stream


def _caller(depth=2):
    f = sys._getframe(depth)
    return "%s:%d (%s)" % (f.f_code.co_filename.rsplit("/", 1)[-1], f.f_lineno, f.f_code.co_name)


def fork(side, origin=None, who=None):
    """`side` waits for everything queued on `origin` (default: the current stream) so far."""
    origin = torch.cuda.current_stream() if origin is None else origin
    side.wait_stream(origin)
    if _ledgers and not _ledgers[-1].is_origin(side):
        _ledgers[-1].open[side.cuda_stream] = (side, who or _caller())


def join(side, into=None):
    """`into` (default: the current stream) waits for everything queued on `side` so far."""
    into = torch.cuda.current_stream() if into is None else into
    into.wait_stream(side)
    if _ledgers:
        led = _ledgers[-1]
        _, who = led.open.pop(side.cuda_stream, (None, None))
        if not led.is_origin(into) and into.cuda_stream not in led.open:
            led.open[into.cuda_stream] = (into, "received the work of the stream forked at %s" % (who or "?"))


def open_streams():
    """[(stream, who)] still open in the capture being audited ([] outside one)."""
    return list(_ledgers[-1].open.values()) if _ledgers else []


_before_capture = []


def before_capture(fn):
    """register fn(device): called by capture() BEFORE the capture begins.  For per-device singletons (flags, counters) that must
    not be born inside a capture: a tensor first made there lives in the graph's pool and holds nothing until the first replay."""
    _before_capture.append(fn)
    return fn


@contextlib.contextmanager
def capture(graph, **kw):
    """torch.cuda.graph(graph, **kw) whose end is audited: RuntimeError (after a rescue join, so that the capture itself ends
    cleanly) when a stream forked inside the body never came back to the capture-origin stream.
    capture_error_mode, when the caller passes none: with a process group alive its watchdog thread polls events; only the capturing
    thread's calls may abort a capture ("thread_local").  Without one, torch's default ("global")."""
    kw.setdefault("capture_error_mode", "thread_local" if dist.is_initialized() else "global")
    if torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
        for fn in _before_capture:
            fn(dev)
    with torch.cuda.graph(graph, **kw):
        led = _Ledger(torch.cuda.current_stream())
        _ledgers.append(led)
        failed = True
        try:
            yield
            failed = False
        finally:
            _ledgers.pop()
            left = list(led.open.values())
            for s, _ in reversed(left):          # rescue: whatever happens next, hipStreamEndCapture sees a joined capture
                led.origin.wait_stream(s)
            if left and not failed:
                raise RuntimeError("hipGraph capture would end with %d unjoined side stream(s): %s -- every stream forked "
                                   "inside a capture must be joined (gm3d_amd.streams.join) before the capture ends"
                                   % (len(left), "; ".join(w for _, w in left)))


def warm_up(fn, iters, device=None):
    """fn() `iters` times on a fresh side stream that waits for the current stream and is waited for by it: the eager iterations
    before a capture (lazy initialisation, library workspaces, code objects).  The caller synchronises."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(iters):
            fn()
    torch.cuda.current_stream().wait_stream(side)


class SideStage:
    """A producer (one workgroup per cloud, most CUs idle: the fine-tune step's point sampling, Point-M2AE's grouping) captured as its
    own graph and replayed on a second stream for the NEXT batch while the caller's training graph of the current batch runs.  A call:
    take(batch, static_in); the caller's copy of the producer's outputs into the training graph's inputs; enqueue(next, static_in)
    BEFORE the training graph is replayed, so that the two run side by side.  With no next batch the producer of a batch runs right
    before its training: same results."""

    def __init__(self, device=None):
        self.stream = torch.cuda.Stream(device=device)
        self.ready, self.staged, self.graph = torch.cuda.Event(), False, None

    def capture(self, fn, generator=None):
        """fn() captured on the stage's stream as the producer graph -> fn's result.  generator: registered with this graph only."""
        self.graph = torch.cuda.CUDAGraph()
        if generator is not None:
            self.graph.register_generator_state(generator)
        with capture(self.graph, stream=self.stream):
            return fn()

    def enqueue(self, src, static_in, before_replay=None):
        """On the stage's stream, after everything the current stream has queued so far (the producer of `src`, and the copy that
        consumed the previous staged results): src -> static_in, before_replay() (host work that belongs between the input copy and
        the replay, on this stream), the producer graph, `ready`."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ev)             # before the copy: src's producer runs on the caller's stream
            static_in.copy_(src, non_blocking=True)
            src.record_stream(self.stream)         # src was allocated on the caller's stream: its block must outlive this copy
            if before_replay is not None:
                before_replay()
            self.graph.replay()
            self.ready.record(self.stream)
        self.staged = True

    def take(self, src, static_in, before_replay=None):
        """The current stream waits for `src`'s staged results: produced now if nothing is staged (first call, or no look-ahead given)."""
        if not self.staged:
            self.enqueue(src, static_in, before_replay)
        torch.cuda.current_stream().wait_event(self.ready)
        self.staged = False


class PinnedFeed:
    """Host arrays -> the given device tensors through two alternating pinned images of them, so that the copies are asynchronous (a
    pageable copy would make the host wait for everything queued before it, once per step)."""

    def __init__(self, *tensors):
        self.tensors = tensors
        self._pin = [[torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in tensors] for _ in range(2)]
        self._ev, self._i = [torch.cuda.Event(), torch.cuda.Event()], 0

    def push(self, arrays):
        """numpy arrays, one per tensor -> the device tensors, on the current stream."""
        i, self._i = self._i, self._i ^ 1
        self._ev[i].synchronize()                  # the copies that last read this image (two pushes ago); nothing before its first record
        for pin, dev, arr in zip(self._pin[i], self.tensors, arrays):
            pin.copy_(torch.from_numpy(arr))
            dev.copy_(pin, non_blocking=True)
        self._ev[i].record(torch.cuda.current_stream())


class LookAhead:
    """The loader's items, each through move(item) (to the device), one ahead: while item i is trained, `next` is item i + 1 (None at
    the end)."""

    def __init__(self, loader, move):
        self.loader, self.move, self.next = loader, move, None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        moved = (self.move(item) for item in self.loader)
        cur = next(moved, None)
        while cur is not None:
            self.next = next(moved, None)
            yield cur
            cur = self.next

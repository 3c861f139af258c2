"""Poisoned allocations: run code with every `empty` allocation filled with a value no correct result can absorb.

A buffer made by torch.empty / empty_like / empty_strided / Tensor.new_empty / new_empty_strided is correct only if its producer writes
every element its consumer reads.  Fresh allocator memory is usually zero or an earlier, plausible result, so a consumer that reads one
unwritten element is "right" in a test and wrong in the tenth training step.  `poisoned(pattern)` fills each such allocation before it
is handed out:

    nan    the arithmetic paths: any sum, product or affine epilogue that touches it turns NaN
    +inf   what a max / arg-max / `x > best` cannot ignore (v_max_f32 and every ordered comparison skip a NaN); 0 * inf is NaN as well
    -inf   the same for min / arg-min (Chamfer, KNN, FPS distances)

Integer dtypes get iinfo.max (nan, +inf) or iinfo.min (-inf) -- 255 / 0 for the uint8 arg-max maps --, bool True / False by the same
rule.  Plain Python: nothing here touches a GPU at import."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gm3d_amd") + os.sep
PATTERNS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
# (owner, attribute): the five entry points
ENTRY_POINTS = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"),
                (torch.Tensor, "new_empty_strided"))

SITES = set()      # every gm3d_amd/<file>:<line> that allocated under poison in this process (the coverage tests read it)
_active = [None]


def fill_value(dtype, pattern):
    """what an allocation of `dtype` holds under `pattern`"""
    if pattern not in PATTERNS:
        raise ValueError("pattern must be one of %s, not %r" % (sorted(PATTERNS), pattern))
    if dtype.is_floating_point:
        return PATTERNS[pattern]
    if dtype.is_complex:
        return complex(PATTERNS[pattern], PATTERNS[pattern])
    if dtype == torch.bool:
        return pattern != "-inf"
    info = torch.iinfo(dtype)
    return info.min if pattern == "-inf" else info.max


class Poison:
    """State of one `poisoned` region: `sites` (gm3d_amd/<file>:<line> of the allocations made from inside the package), `recorded` (how
    many allocations those were) and `count` (all allocations poisoned, whoever made them)."""

    def __init__(self, pattern, only=None):
        self.pattern = pattern
        self.only = None if only is None else set(only)
        self.sites = set()
        self.recorded = 0
        self.count = 0

    def _site(self, frame):
        path = os.path.abspath(frame.f_code.co_filename)
        if not path.startswith(PKG):
            return None
        return "gm3d_amd/%s:%d" % (path[len(PKG):].replace(os.sep, "/"), frame.f_lineno)

    def _poison(self, t, frame):
        site = self._site(frame)
        if site is not None:
            self.sites.add(site)
            SITES.add(site)
            self.recorded += 1
        if self.only is not None and site not in self.only:
            return t
        if isinstance(t, torch.Tensor) and t.numel() > 0:
            t.detach().fill_(fill_value(t.dtype, self.pattern))
            if t.is_cuda:
                # the fill runs on the current stream; a side stream forked BEFORE this allocation (the parallel inference chains
                # write their rows of one output buffer made after the fork) is ordered behind nothing of it and could write first,
                # to be overwritten by the poison.  No capture can be running (refused at entry), so waiting is allowed.
                torch.cuda.synchronize(t.device)
            self.count += 1
        return t


def _wrap(orig, state):
    def wrapper(*args, **kwargs):
        return state._poison(orig(*args, **kwargs), sys._getframe(1))
    wrapper.__name__ = getattr(orig, "__name__", "empty")
    wrapper.__wrapped__ = orig
    return wrapper


class poisoned:
    """with poisoned(pattern) as state: every allocation of the five entry points is filled with `pattern`'s value until the block ends;
    the originals come back exactly, also after an exception.  `state` (also `.state` of the object afterwards) is the region's Poison.
    only=: an iterable of sites ("gm3d_amd/ops.py:103"): poison those allocations alone (all are still recorded) -- for finding which
    buffer a failing case reads.  Not re-entrant, and refused while a stream is capturing: a captured graph stays what it is (replay is
    covered by the graph tests)."""

    def __init__(self, pattern, only=None):
        fill_value(torch.float32, pattern)
        self.state = Poison(pattern, only)
        self._saved = None

    def __enter__(self):
        if _active[0] is not None:
            raise RuntimeError("poisoned() is already active")
        if torch.cuda.is_available() and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("poisoned() must not be entered while a stream is capturing")
        _active[0] = self.state
        self._saved = []
        try:
            for owner, name in ENTRY_POINTS:
                own = name in vars(owner)      # Tensor inherits its methods from the C base class: leave nothing of ours there
                orig = getattr(owner, name)
                setattr(owner, name, _wrap(orig, self.state))
                self._saved.append((owner, name, own, orig))
        except BaseException:
            self._restore()
            raise
        return self.state

    def _restore(self):
        for owner, name, own, orig in reversed(self._saved):
            if own:
                setattr(owner, name, orig)
            else:
                delattr(owner, name)
        self._saved = None
        _active[0] = None

    def __exit__(self, *exc):
        self._restore()
        return False


# ------------------------------------------------------------------------------------------------------------------ comparing results
def leaves(x, path=""):
    """nested tuples / lists / dicts -> [(path, leaf)] in a fixed order"""
    if isinstance(x, dict):
        return [kv for k in sorted(x, key=str) for kv in leaves(x[k], "%s[%r]" % (path, k))]
    if isinstance(x, (tuple, list)):
        return [kv for i, v in enumerate(x) for kv in leaves(v, "%s[%d]" % (path, i))]
    return [(path, x)]


def _exempt_mask(exempt, path, t):
    """exempt: {part of a leaf's path: True | bool tensor (True = the operation defines this element as zero or NaN)}"""
    for key, m in (exempt or {}).items():
        if key in path:
            if m is True:
                return torch.ones_like(t, dtype=torch.bool)
            return m.to(t.device).expand_as(t)
    return None


def assert_same(plain, pois, name, exempt=None):
    """plain / pois: the same operation's results (nested tuples, lists, dicts of tensors) without and with poison.  Same structure,
    shapes and dtypes; the plain result finite and (floating tensors) not all zero outside `exempt` -- the elements the operation itself
    defines as zero or NaN, stated by the caller --; the two bit-identical (torch.equal; NaN at the same places, which the finiteness
    check confines to `exempt`).  An integer map may be all zero by right (the arg-max over one candidate), so only equality is asked
    of those."""
    lp, lq = leaves(plain, name), leaves(pois, name)
    assert [p for p, _ in lp] == [p for p, _ in lq], "%s: the two results differ in structure" % name
    assert lp, "%s: nothing to compare" % name
    for (path, a), (_, b) in zip(lp, lq):
        if not isinstance(a, torch.Tensor):
            assert not isinstance(b, torch.Tensor) and a == b, "%s: %r vs %r" % (path, a, b)
            continue
        assert isinstance(b, torch.Tensor), "%s: tensor vs %r" % (path, type(b))
        assert a.shape == b.shape and a.dtype == b.dtype, "%s: %s %s vs %s %s" % (path, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
        if a.numel() == 0:
            continue
        a, b = a.detach(), b.detach()
        if not (a.dtype.is_floating_point or a.dtype.is_complex):
            assert torch.equal(a, b), "%s: %d of %d elements differ under poison" % (path, int((a != b).sum()), a.numel())
            continue
        mask = _exempt_mask(exempt, path, a)
        live = a if mask is None else a[~mask]
        assert bool(torch.isfinite(live).all()), "%s: the plain result is not finite" % path
        assert live.numel() == 0 or bool((live != 0).any()), "%s: the plain result is all zero (a vacuous case)" % path
        an, bn = a.isnan(), b.isnan()
        bad = (an != bn) | (a.masked_fill(an, 0) != b.masked_fill(bn, 0))
        assert not bool(bad.any()), "%s: %d of %d elements differ under poison (first at flat index %d)" % (
            path, int(bad.sum()), a.numel(), int(bad.flatten().nonzero()[0]))


def assert_within(plain, pois, name, tol):
    """The weaker form, ONLY for a tensor whose two plain runs already differ bitwise (an atomic scatter): the poisoned tensor within
    tol * max|plain| of the plain one -- the form of the bar the operation's own test holds it to --, non-finite nowhere the plain one
    is finite."""
    lp, lq = leaves(plain, name), leaves(pois, name)
    assert [p for p, _ in lp] == [p for p, _ in lq], "%s: the two results differ in structure" % name
    for (path, a), (_, b) in zip(lp, lq):
        assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype.is_floating_point, path
        assert a.shape == b.shape and a.dtype == b.dtype, path
        a, b = a.detach().double(), b.detach().double()
        assert not bool((~torch.isfinite(b) & torch.isfinite(a)).any()), "%s: non-finite under poison where the plain run is finite" % path
        ok = torch.isfinite(a)
        assert bool(ok.any()) and bool((a[ok] != 0).any()), "%s: the plain result holds no finite non-zero value" % path
        err = float((a[ok] - b[ok]).abs().max())
        scale = max(float(a[ok].abs().max()), 1e-6)
        assert err <= tol * scale, "%s: error %.3e of scale %.3e under poison, bar %.1e" % (path, err, scale, tol)


def scan_sites():
    """every gm3d_amd/<file>:<line> whose line names one of the entry points (code lines only: comments and docstrings allocate nothing)"""
    import io
    import tokenize
    out = {}
    words = ("torch.empty", "new_empty", "empty_like", "empty_strided")
    for fn in sorted(os.listdir(PKG)):
        if not fn.endswith(".py"):
            continue
        with open(os.path.join(PKG, fn)) as f:
            src = f.read()
        code = {}
        for tok in tokenize.generate_tokens(io.StringIO(src).readline):
            if tok.type in (tokenize.COMMENT, tokenize.STRING, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT):
                continue
            code.setdefault(tok.start[0], []).append(tok.string)
        for ln, toks in code.items():
            text = "".join(toks)
            if any(w in text for w in words):
                out["gm3d_amd/%s:%d" % (fn, ln)] = text
    return out


# ------------------------------------------------------------------------------------------------------------------ coverage
CASES = {}         # test module -> (cases that ran to their end, cases it has): filled by the two GPU modules
HOT = ("gm3d_amd/gemm.py", "gm3d_amd/embed.py", "gm3d_amd/fused.py", "gm3d_amd/ops.py", "gm3d_amd/heads.py", "gm3d_amd/attention.py")
UNREACHED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poison_unreached.json")


def coverage(complete):
    """The coverage condition over SITES, the union of what this process poisoned.  tests/golden/poison_unreached.json names the
    allocation lines no case reaches, {site: {"reason": ..., "switch": ...}}: at most 15 % of the scanned lines; none in gemm / embed / attention /
    fused / ops / heads unless behind a switch that is off by default, which is named; none that IS reached (the list cannot rot).
    complete (every poison case of the process ran): every scanned line is reached or listed.  -> (scanned, reached, listed) counts."""
    with open(UNREACHED) as f:
        listed = json.load(f)
    scanned = scan_sites()
    reached = {s for s in SITES if s in scanned}
    assert all(isinstance(v, dict) and v.get("reason") for v in listed.values()), "every listed site carries a one-line reason"
    stale = sorted(s for s in listed if s not in scanned)
    assert not stale, "listed, but not an allocation line: %s" % stale
    rotten = sorted(s for s in listed if s in reached)
    assert not rotten, "listed as unreached, but reached: %s" % rotten
    assert len(listed) <= 0.15 * len(scanned), "%d of %d sites listed: more than 15 %%" % (len(listed), len(scanned))
    for s, v in listed.items():
        if s.split(":")[0] in HOT:
            assert v.get("switch"), "%s is in a hot-path file: only a site behind a switch that is off by default may be listed" % s
    if complete:
        missing = sorted(s for s in scanned if s not in reached and s not in listed)
        assert not missing, "%d allocation sites neither reached under poison nor listed:\n%s" % (
            len(missing), "\n".join("%s  %s" % (s, scanned[s][:110]) for s in missing))
    return len(scanned), len(reached), len(listed)

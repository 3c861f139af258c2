"""The poison harness (tests/poison.py) tested on CPU tensors: every entry point, dtype class and pattern; exact restoration; site
recording; and the two toys that pin why there are three patterns -- a max-reducing finish over a partial buffer with one unwritten row
is caught under +inf and MISSED under nan, a sum-reducing one is caught under all three."""
import math
import os

import pytest
import torch

from tests import poison
from tests.poison import assert_same, poisoned

PATTERNS = ["nan", "+inf", "-inf"]
ENTRIES = {
    "empty": lambda dt: torch.empty(3, 5, dtype=dt),
    "empty_like": lambda dt: torch.empty_like(torch.zeros(3, 5, dtype=dt)),
    "empty_strided": lambda dt: torch.empty_strided((3, 5), (5, 1), dtype=dt),
    "new_empty": lambda dt: torch.zeros(2, dtype=dt).new_empty(3, 5),
    "new_empty_strided": lambda dt: torch.zeros(2, dtype=dt).new_empty_strided((3, 5), (5, 1)),
}
DTYPES = [torch.float64, torch.float32, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.uint8, torch.bool]


def _expect(t, dt, pattern):
    if dt.is_floating_point:
        if pattern == "nan":
            return bool(t.isnan().all())
        return bool((t == (math.inf if pattern == "+inf" else -math.inf)).all())
    if dt == torch.bool:
        return bool((t == (pattern != "-inf")).all())
    info = torch.iinfo(dt)
    return bool((t == (info.min if pattern == "-inf" else info.max)).all())


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_entry_point_is_poisoned_for_every_dtype_class(entry, pattern):
    with poisoned(pattern) as ps:
        got = [(dt, ENTRIES[entry](dt)) for dt in DTYPES]
    assert ps.count == len(DTYPES)
    for dt, t in got:
        assert t.dtype == dt and tuple(t.shape) == (3, 5)
        assert _expect(t, dt, pattern), (entry, dt, pattern, t)


def test_uint8_gets_255_and_0():
    for pattern, want in (("nan", 255), ("+inf", 255), ("-inf", 0)):
        with poisoned(pattern):
            t = torch.empty(4, dtype=torch.uint8)
        assert t.tolist() == [want] * 4


def test_keyword_forms_views_and_leaves_that_require_grad():
    with poisoned("+inf") as ps:
        a = torch.empty((2, 3), dtype=torch.float32, device="cpu")
        b = torch.empty(2, 3, requires_grad=True)
        c = torch.empty_like(a, dtype=torch.int32)
        d = torch.empty(0, 7)
        e = torch.empty((), dtype=torch.float32)
    assert bool((a == math.inf).all()) and bool((b == math.inf).all()) and b.requires_grad and b.is_leaf
    assert c.dtype == torch.int32 and bool((c == torch.iinfo(torch.int32).max).all())
    assert d.numel() == 0 and float(e) == math.inf
    assert ps.count == 4          # the empty tensor holds nothing to poison


def _originals():
    return [(owner, name, getattr(owner, name), name in vars(owner)) for owner, name in poison.ENTRY_POINTS]


def _assert_restored(before):
    for owner, name, fn, own in before:
        assert getattr(owner, name) is fn, name
        assert (name in vars(owner)) == own, name
    assert not bool(torch.empty(64, dtype=torch.float64).isnan().all())       # and nothing fills any more


def test_originals_come_back_after_normal_exit():
    before = _originals()
    with poisoned("nan"):
        for owner, name, fn, _ in before:
            assert getattr(owner, name) is not fn
    _assert_restored(before)


def test_originals_come_back_after_an_exception():
    before = _originals()
    with pytest.raises(ZeroDivisionError):
        with poisoned("-inf"):
            torch.empty(3)
            1 / 0
    _assert_restored(before)
    with poisoned("nan") as ps:                # and the harness can be entered again
        torch.empty(3)
    assert ps.count == 1


def test_not_reentrant_and_unknown_pattern():
    before = _originals()
    with poisoned("nan"):
        with pytest.raises(RuntimeError):
            with poisoned("+inf"):
                pass
    _assert_restored(before)
    with pytest.raises(ValueError):
        with poisoned("zero"):
            pass
    _assert_restored(before)


def test_refuses_to_start_inside_a_capture(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    before = _originals()
    with pytest.raises(RuntimeError, match="capturing"):
        with poisoned("nan"):
            pass
    _assert_restored(before)


# ------------------------------------------------------------------------------------------------------------------ site recording
def test_sites_name_the_calling_line_inside_the_package(tmp_path, monkeypatch):
    """A caller counts when its file lies under gm3d_amd/: a module written there for the test (under a temporary root) is recorded by
    line, this test file is not."""
    pkg = tmp_path / "gm3d_amd"
    pkg.mkdir()
    src = ("import torch\n"                                   # 1
           "def f(x):\n"                                      # 2
           "    a = torch.empty(3)\n"                         # 3
           "    b = x.new_empty(2,\n"                         # 4
           "                    2)\n"                         # 5
           "    c = [torch.empty_like(t) for t in (a, b)]\n"  # 6
           "    return a, b, c\n")
    path = pkg / "toy_alloc.py"
    path.write_text(src)
    monkeypatch.setattr(poison, "PKG", str(pkg) + os.sep)
    ns = {}
    exec(compile(src, str(path), "exec"), ns)
    had = set(poison.SITES)
    with poisoned("nan") as ps:
        torch.empty(5)                      # from tests/: poisoned, not recorded
        ns["f"](torch.zeros(1))
    assert ps.sites == {"gm3d_amd/toy_alloc.py:3", "gm3d_amd/toy_alloc.py:4", "gm3d_amd/toy_alloc.py:6"}
    assert ps.recorded == 4 and ps.count == 5
    assert poison.SITES - had == ps.sites
    poison.SITES.difference_update(ps.sites)
    monkeypatch.undo()
    scanned = poison.scan_sites()
    assert scanned and all(k.startswith("gm3d_amd/") for k in scanned)


def test_site_filter_poisons_the_named_site_alone(tmp_path, monkeypatch):
    pkg = tmp_path / "gm3d_amd"
    pkg.mkdir()
    src = "import torch\ndef f():\n    a = torch.empty(3, dtype=torch.int32)\n    b = torch.empty(3, dtype=torch.int32)\n    return a, b\n"
    monkeypatch.setattr(poison, "PKG", str(pkg) + os.sep)
    ns = {}
    exec(compile(src, str(pkg / "toy_filter.py"), "exec"), ns)
    with poisoned("+inf", only=["gm3d_amd/toy_filter.py:4"]) as ps:
        a, b = ns["f"]()
    big = torch.iinfo(torch.int32).max
    assert b.tolist() == [big] * 3 and ps.count == 1 and ps.recorded == 2
    assert ps.sites == {"gm3d_amd/toy_filter.py:3", "gm3d_amd/toy_filter.py:4"}
    poison.SITES.difference_update(ps.sites)


def test_scan_skips_comments_and_docstrings(tmp_path, monkeypatch):
    pkg = tmp_path / "gm3d_amd"
    pkg.mkdir()
    (pkg / "m.py").write_text('"""torch.empty in a docstring"""\nimport torch\n# torch.empty in a comment\nx = torch.empty(1)  # here\n'
                              'y = x.new_empty(\n    2)\nz = torch.empty_like(x); w = torch.empty_strided((1,), (1,))\n')
    monkeypatch.setattr(poison, "PKG", str(pkg) + os.sep)
    assert sorted(poison.scan_sites()) == ["gm3d_amd/m.py:4", "gm3d_amd/m.py:5", "gm3d_amd/m.py:7"]


# ------------------------------------------------------------------------------------------------------------------ the toys
def toy_max_finish(x, n):
    """WRONG on purpose: the host sizes the partial buffer one row larger than the grid writes, the finish max-reduces all of it."""
    part = torch.empty(n + 1, x.shape[1], dtype=x.dtype)
    for i in range(n):
        part[i] = x[i * 4:(i + 1) * 4].amax(0)
    best = part[0].clone()
    for i in range(1, n + 1):                 # the kernels' `x > best`: an ordered comparison, false for a NaN
        best = torch.where(part[i] > best, part[i], best)
    return best


def toy_sum_finish(x, n):
    """WRONG on purpose in the same way, with a sum."""
    part = torch.empty(n + 1, x.shape[1], dtype=x.dtype)
    for i in range(n):
        part[i] = x[i * 4:(i + 1) * 4].sum(0)
    return part.sum(0)


def _plain_with_stale_zero_row(toy, x, n, monkeypatch):
    """the plain run as the caching allocator typically serves it: the unwritten row holds zeros (or an earlier, smaller result)"""
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **k))
        return toy(x, n)


def _caught(toy, pattern, monkeypatch):
    x = torch.rand(12, 6, generator=torch.Generator().manual_seed(0)) + 0.5
    plain = _plain_with_stale_zero_row(toy, x, 3, monkeypatch)
    with poisoned(pattern) as ps:
        got = toy(x, 3)
    assert ps.count >= 1
    try:
        assert_same(plain, got, "toy")
    except AssertionError:
        return True
    return False


def test_max_finish_over_an_unwritten_row_is_caught_by_plus_inf_and_missed_by_nan(monkeypatch):
    assert _caught(toy_max_finish, "+inf", monkeypatch)
    assert not _caught(toy_max_finish, "nan", monkeypatch), "an ordered comparison ignores NaN: this is why NaN alone is not enough"
    assert not _caught(toy_max_finish, "-inf", monkeypatch)      # -inf is the pattern of the min reductions, not this one


def test_min_finish_needs_minus_inf(monkeypatch):
    def toy_min_finish(x, n):
        part = torch.empty(n + 1, x.shape[1], dtype=x.dtype)
        for i in range(n):
            part[i] = x[i * 4:(i + 1) * 4].amin(0)
        best = part[0].clone()
        for i in range(1, n + 1):
            best = torch.where(part[i] < best, part[i], best)
        return best

    x = torch.rand(12, 6, generator=torch.Generator().manual_seed(1)) + 0.5
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", lambda *a, **k: torch.full(a, 9.0, **k))      # a stale, larger row: harmless to a min
        plain = toy_min_finish(x, 3)
    seen = {}
    for pattern in PATTERNS:
        with poisoned(pattern):
            got = toy_min_finish(x, 3)
        try:
            assert_same(plain, got, "toy")
            seen[pattern] = False
        except AssertionError:
            seen[pattern] = True
    assert seen == {"nan": False, "+inf": False, "-inf": True}


@pytest.mark.parametrize("pattern", PATTERNS)
def test_sum_finish_over_an_unwritten_row_is_caught_by_every_pattern(pattern, monkeypatch):
    assert _caught(toy_sum_finish, pattern, monkeypatch)


def test_a_correct_finish_passes_under_every_pattern():
    def good(x, n):
        part = torch.empty(n, x.shape[1], dtype=x.dtype)
        arg = torch.empty(n, x.shape[1], dtype=torch.uint8)
        for i in range(n):
            part[i], a = x[i * 4:(i + 1) * 4].max(0)
            arg[i] = a.to(torch.uint8)
        return {"max": part.amax(0), "arg": arg}

    x = torch.rand(12, 6, generator=torch.Generator().manual_seed(2)) + 0.5
    plain = good(x, 3)
    for pattern in PATTERNS:
        with poisoned(pattern) as ps:
            got = good(x, 3)
        assert ps.count == 2
        assert_same(plain, got, "good")


# ------------------------------------------------------------------------------------------------------------------ assert_same
def test_assert_same_rules():
    a = {"y": torch.tensor([1.0, 2.0]), "i": (torch.tensor([0, 0]), None)}
    assert_same(a, {"y": torch.tensor([1.0, 2.0]), "i": (torch.tensor([0, 0]), None)}, "ok")
    for bad in ({"y": torch.tensor([1.0, 2.5]), "i": (torch.tensor([0, 0]), None)},          # a value
                {"y": torch.tensor([1.0, 2.0]), "i": (torch.tensor([0, 1]), None)},          # an index
                {"y": torch.tensor([1.0, 2.0], dtype=torch.float64), "i": (torch.tensor([0, 0]), None)},
                {"y": torch.tensor([[1.0, 2.0]]), "i": (torch.tensor([0, 0]), None)},
                {"y": torch.tensor([1.0, 2.0])}):
        with pytest.raises(AssertionError):
            assert_same(a, bad, "bad")
    with pytest.raises(AssertionError, match="all zero"):
        assert_same(torch.zeros(3), torch.zeros(3), "vacuous")
    with pytest.raises(AssertionError, match="not finite"):
        assert_same(torch.tensor([1.0, math.nan]), torch.tensor([1.0, math.nan]), "nan")
    # elements the operation defines as zero or NaN are stated by the caller, and must still agree
    dead = torch.tensor([False, True])
    assert_same((torch.tensor([1.0, math.nan]),), (torch.tensor([1.0, math.nan]),), "r", exempt={"[0]": dead})
    assert_same(torch.zeros(3), torch.zeros(3), "z", exempt={"z": True})
    with pytest.raises(AssertionError):
        assert_same((torch.tensor([1.0, math.nan]),), (torch.tensor([1.0, 0.0]),), "r", exempt={"[0]": dead})
    with pytest.raises(AssertionError):
        assert_same((torch.tensor([1.0, 0.0]),), (torch.tensor([1.0, math.inf]),), "r", exempt={"[0]": dead})


def test_assert_within_is_the_bar_and_no_new_non_finite():
    a = torch.tensor([1.0, 2.0, math.nan])
    poison.assert_within(a, torch.tensor([1.0 + 1e-7, 2.0, math.nan]), "w", 1e-6)
    with pytest.raises(AssertionError):
        poison.assert_within(a, torch.tensor([1.0 + 1e-3, 2.0, math.nan]), "w", 1e-6)
    with pytest.raises(AssertionError):
        poison.assert_within(a, torch.tensor([math.inf, 2.0, math.nan]), "w", 1e-6)
    with pytest.raises(AssertionError):
        poison.assert_within(torch.zeros(2), torch.zeros(2), "w", 1e-6)

"""No GPU: the inputs and the bars of tests/test_gpu_mattn_sparse.py, checked before a kernel sees them.

Structure: every mask is symmetric and really contains what it exists for -- a wave-blocked key tile BEFORE a live one
(blockdiag, anti), a 32-query tile whose rows disagree about whether a key tile is live (sparse, radius), rows without any
allowed key (padding).  These are conditions on the inputs: a seed that misses one is replaced (mattn_ref.seed_of).

Error measurement: for every GPU case the restatement of its mode (mattn_ref.emulate_bf16 for bf16, mattn_ref.restate_f32 for
f32) is compared with the fp64 reference in the metrics of the GPU test.  It must sit within HALF the bar the case uses -- a bar
the rounding of the number format alone nearly exhausts would test nothing -- and the table must equal the committed
tests/golden/mattn_sparse_bars.json, from which the GPU test takes the `amp` bars.
Regenerate: python -m tests.test_mattn_ref_cpu"""
import json

import pytest
import torch

from tests import mattn_ref as R

TABLE = R.TABLE
KIND_T = sorted({(c.kind, c.T, c.B) for c in R.cases()})


@pytest.mark.parametrize("kind,T,B", KIND_T)
def test_mask_structure(kind, T, B):
    c = R.Case("base", kind, T, 16, B, "f32")
    raw = R.masks(kind, B, T, R.seed_of(c))
    n = R.pad_lengths(B, T)
    mask = R.pad(raw, n)
    assert raw.dtype == torch.bool and tuple(raw.shape) == (B, T, T)
    assert torch.equal(raw, raw.transpose(1, 2)) and torch.equal(mask, mask.transpose(1, 2))
    assert not raw[:, torch.arange(T), torch.arange(T)].any() or kind == "anti"
    for b in range(B):
        assert torch.equal(mask[b, :n[b], :n[b]], raw[b, :n[b], :n[b]])
        assert mask[b, n[b]:].all() and mask[b, :, n[b]:].all()
    if T > 1:
        assert mask.all(dim=2).any(), "padding must produce rows without an allowed key"
        assert (~mask.all(dim=2)).any()
    blocked, NT = R.tile_structure(raw[0])                           # cloud 0 is not padded (n[0] = T)
    wave = blocked.view(NT, -1, NT).all(dim=1) if T % 32 == 0 else torch.stack(
        [blocked[32 * t:32 * t + 32].all(dim=0) for t in range(NT)])    # (query tile, key tile): blocked for the whole wave
    if kind in ("blockdiag", "anti") and NT > 1:
        first_live = (~wave).float().argmax(dim=1)
        last_live = NT - 1 - (~wave).flip(1).float().argmax(dim=1)
        assert (~wave).any(dim=1).all()
        assert any(wave[t, :last_live[t]].any() for t in range(NT)), "no wave-blocked tile ahead of a live one"
        assert (first_live > 0).any()                                # some wave starts with m = -inf over skipped tiles
    if kind in ("sparse", "radius") and T > 32:
        mixed = [(t, kt) for t in range(NT) for kt in range(NT)
                 if blocked[32 * t:32 * t + 32, kt].any() and not blocked[32 * t:32 * t + 32, kt].all()]
        assert mixed, "no query tile whose rows disagree about a key tile"
        # and a lane whose running maximum is still -inf after a tile its wave did compute (the two `mn == -INFINITY` guards);
        # at T = 33 the only row with its diagonal outside tile 0 is a wave of its own
        first = (~blocked).float().argmax(dim=1)                     # first live key tile of every row (each row has its diagonal)
        assert NT == 2 or any(not wave[i // 32, :first[i]].all() for i in range(T)), "no lane idles through a computed tile"
    if kind == "anti":
        assert raw[0, 0, :32 * (NT - 1)].all() and not raw[0, 0, 32 * (NT - 1):].all()    # tile 0 lives on the last tile alone


def measure(c):
    """The restatement of the case's mode against fp64 -> ({metric: error}, dead rows exactly zero)."""
    qkv, dout, mask, clean = R.inputs(c)
    scale = c.hd ** -0.5
    q64, d64 = clean.double(), dout.double()
    ref = R.reference_grad(q64, mask, R.H, c.hd, scale, d64)
    got = (R.emulate_bf16 if c.dtype == "bf16" else R.restate_f32)(qkv, mask, R.H, c.hd, scale, dout)
    assert all(bool(torch.isfinite(t).all()) for t in got + ref)
    return R.errors(got, ref, q64, d64, mask, R.H, c.hd, c.dtype), R.dead_rows_are_zero(*got, mask, R.H, c.hd)


def generate():
    return {R.case_id(c): measure(c)[0] for c in R.cases()}


@pytest.fixture(scope="module")
def committed():
    with open(TABLE) as f:
        return json.load(f)


def test_reference_is_the_formula_of_the_dense_test():
    """reference() against an explicit per-row loop in fp64 (one head, small T), lse included."""
    c = R.Case("base", "sparse", 33, 16, 4, "f32")
    qkv, _, mask, _ = R.inputs(c)
    out, lse = R.reference(qkv.double(), mask, R.H, c.hd, 0.25)
    x = qkv.double().view(c.B, c.T, 3, R.H, c.hd)
    for b, h in ((0, 0), (1, 5), (2, 3)):
        for i in range(c.T):
            keys = (~mask[b, i]).nonzero().flatten()
            if len(keys) == 0:
                assert float(lse[b, h, i]) == 0.0 and not out[b, i].any()
                continue
            s = (x[b, keys, 1, h] @ x[b, i, 0, h]) * 0.25
            w = torch.exp(s - s.max())
            assert torch.allclose(out[b, i, h * c.hd:(h + 1) * c.hd], (w / w.sum()) @ x[b, keys, 2, h], rtol=1e-12, atol=1e-14)
            assert abs(float(lse[b, h, i]) - float(s.max() + torch.log(w.sum()))) < 1e-12


def test_restatements_sit_within_half_of_every_bar_and_match_the_committed_table(committed):
    ids = [R.case_id(c) for c in R.cases()]
    assert sorted(committed) == sorted(ids)
    print("\n%-38s %s" % ("case", "  ".join("%-9s" % m for m in ("out", "lse", "dq", "dk", "dv"))))
    for c in R.cases():
        got, dead_ok = measure(c)
        cid = R.case_id(c)
        print("%-38s %s" % (cid, "  ".join("%-9.2e" % got.get(m, got.get(m + "_zero", float("nan")))
                                          for m in ("out", "lse", "dq", "dk", "dv"))))
        assert dead_ok, cid
        bar = R.bars(c, committed[cid])
        assert sorted(got) == sorted(committed[cid]), cid
        for k, e in got.items():
            assert e <= 0.5 * bar[k], (cid, k, e, bar[k])
            # the committed figure is this measurement; a BLAS that sums in another order moves a maximum of rounding errors by
            # tens of per cent, never by a factor of two (below 1e-3 of the bar the figure is noise)
            want = committed[cid][k]
            assert abs(e - want) <= 0.5 * max(e, want) + 1e-3 * R.BARS[c.dtype][k], (cid, k, e, want)


if __name__ == "__main__":
    table = generate()
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")

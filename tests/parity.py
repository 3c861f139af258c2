"""Comparison helpers of the bf16 parity tests (tests/test_gpu_bf16_parity.py, tests/test_gpu_b128.py): rel-L2 / cosine, a
ledger of (tensor, error, bar) rows that fails naming the worst offenders, and a tile check for LOCALIZED errors.

Why the tile check: a whole-tensor rel-L2 averages one wrong tile away.  The round-4 attn_qkv_fwd race left one (cloud, head) tile
of the attention input wrong by up to 0.25 -- at B=128 that is 1/768 of the tensor, a rel-L2 change far inside any bf16 bar.  The
error of a correct bf16 computation is spread evenly: no block's error stands far above the median block's.  So each block's
RMS error, measured in units of the block's own scale (its reference RMS, but at least the median block's RMS, so that nearly-zero
blocks are not judged by their own noise), is compared with TILE_FACTOR x the median block's value.

Plain module (not a conftest): imported by the tests that use it."""
import math

import torch

TILE_FACTOR = 10.0      # a block may stand this far above the tensor's median block before it is called localized
TILE = 64


def _d(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def rel_l2(got, ref):
    """||got - ref|| / ||ref|| in float64."""
    got, ref = _d(got), _d(ref)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def cosine(got, ref):
    got, ref = _d(got).flatten(), _d(ref).flatten()
    return float(got @ ref / (got.norm() * ref.norm()).clamp_min(1e-300))


def _blocks(t, kind, stride=1):
    """-> list of (label, index tuple) covering `t`.
    kind "weight": t viewed as 2-D [out, in] (trailing dims folded), TILE x TILE blocks (ragged edges kept).  stride > 1: `t` is
    the sub-grid w[::stride, ::stride] of such a weight: its (TILE/stride)^2 blocks are the samples of the weight's TILE x TILE
    blocks, and the labels name the weight's rows and columns;
    kind "act": t is [B, T, C] (or [B, C]): one block per cloud, and one per (cloud, TILE-column head slice)."""
    if kind == "weight":
        out, inn, bs = t.shape[0], int(t.numel() // t.shape[0]), TILE // stride
        return [("[%d:%d, %d:%d]" % (r * stride, min(r + bs, out) * stride, c * stride, min(c + bs, inn) * stride),
                 (slice(r, r + bs), slice(c, c + bs))) for r in range(0, out, bs) for c in range(0, inn, bs)]
    if kind == "act":
        B, C = t.shape[0], t.shape[-1]
        blocks = [("cloud %d" % b, (b,)) for b in range(B)]
        if C > TILE:
            blocks += [("cloud %d cols %d:%d" % (b, c, min(c + TILE, C)), (b, Ellipsis, slice(c, c + TILE)))
                       for b in range(B) for c in range(0, C, TILE)]
        return blocks
    raise ValueError(kind)


def tile_scores(got, ref, kind, floor=0.0, stride=1):
    """-> [(score, label, rms_err)] sorted worst first; score = block error / (TILE_FACTOR x median block error), so a
    score > 1 is a localized error.  Blocks whose RMS error is <= `floor` (absolute) score 0.  stride: see _blocks."""
    got, ref = _d(got), _d(ref)
    if kind == "weight":
        got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    blocks = _blocks(ref, kind, stride)
    err = [float((got[ix] - ref[ix]).pow(2).mean().sqrt()) for _, ix in blocks]
    scale = [float(ref[ix].pow(2).mean().sqrt()) for _, ix in blocks]
    groups = {}         # per-cloud blocks and per-slice blocks are judged against medians of their own kind
    for i, (label, _) in enumerate(blocks):
        groups.setdefault("cols" in label, []).append(i)
    out = []
    for idx in groups.values():
        s_med = float(torch.tensor([scale[i] for i in idx]).median())
        norm = [err[i] / max(scale[i], s_med, 1e-300) for i in idx]
        n_med = float(torch.tensor(norm).median())
        for i, n in zip(idx, norm):
            score = 0.0 if err[i] <= floor else n / max(TILE_FACTOR * n_med, 1e-300)
            out.append((score, blocks[i][0], err[i]))
    out.sort(key=lambda r: -r[0])
    return out


class Ledger:
    """Collects one row per check: (name, measured, bar).  `assert_ok` fails if any row is over its bar, and the message lists
    the six worst rows by measured/bar, so that a miss names its tensor (or block)."""

    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, name, measured, bar, higher_is_better=False):
        """ratio = measured / bar (or, for higher_is_better quantities such as a cosine, (1 - measured) / (1 - bar))."""
        measured, bar = float(measured), float(bar)
        if higher_is_better:
            ratio = (1.0 - measured) / max(1.0 - bar, 1e-300)
        else:
            ratio = measured / bar if bar > 0 else (0.0 if measured == 0 else math.inf)
        if math.isnan(measured):
            ratio = math.inf
        self.rows.append((ratio, name, measured, bar))
        return ratio

    def rel(self, name, got, ref, bar):
        """rel-L2 of `got` against `ref` within `bar`."""
        return self.add(name + " rel-L2", rel_l2(got, ref), bar)

    def cos(self, name, got, ref, bar=0.999):
        return self.add(name + " cosine", cosine(got, ref), bar, higher_is_better=True)

    def tiles(self, name, got, ref, kind, floor=0.0, stride=1):
        """the worst block of `got` vs `ref` (see tile_scores); its score is already a ratio to the bar."""
        score, label, err = tile_scores(got, ref, kind, floor, stride)[0]
        self.rows.append((score, "%s tile %s (rms err %.3g)" % (name, label, err), score, 1.0))
        return score

    def worst(self, n=6):
        return sorted(self.rows, key=lambda r: -r[0])[:n]

    def max_ratio(self, prefix=""):
        return max((r[0] for r in self.rows if r[1].startswith(prefix)), default=0.0)

    def report(self, n=6):
        return "%s: %d checks, worst measured/bar:\n" % (self.title, len(self.rows)) + "\n".join(
            "  %8.3f  %s  (%.3e vs bar %.3e)" % (r, name, m, b) for r, name, m, b in self.worst(n))

    def assert_ok(self):
        bad = [r for r in self.rows if not r[0] <= 1.0]
        assert not bad, "%d of %d checks over their bar. %s" % (len(bad), len(self.rows), self.report())

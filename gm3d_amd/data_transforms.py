"""Point-cloud augmentations on the device: the reference's Point-MAE_SA3D/datasets/data_transforms.py (P/ below), any chain of
them as ONE launch (gm3d_augment, csrc/augment.hip).

The reference applies each transform cloud by cloud on the host side of the stream: np.random draws, one host-to-device copy per
cloud, `.tolist()` in the dropout, up to two `torch.max` synchronisations per cloud in the flip -- none of which a hipGraph can
record.  Here a `Compose` draws everything the chain needs in at most three calls on one generator (torch.rand(B, D), torch.rand(B, N)
if a dropout is in the chain, torch.randn(B, N, 3) if a jitter is) and issues one launch that applies the whole chain in place, so
it can be captured with the step and replays with fresh draws:

    from gm3d_amd import data_transforms as T, engine_pretrain_point_mae as EP
    EP.train_transforms = T.Compose([T.PointcloudScale(), T.PointcloudTranslate(), T.PointcloudJitter(),
                                     T.PointcloudRandomInputDropout(), T.RandomHorizontalFlip()])

Every object is callable as `t(pc, draws=None, generator=None)`, modifies pc (B,N,3) in place and returns it, like the reference's.
`draws` injects an op's random quantities (parity tests); for a Compose it is a list aligned with the chain whose None entries are
drawn live:

    PointcloudRotate              (B,) the uniform u of angle = 2 pi u
    PointcloudScale               (B,3) the final scales
    PointcloudTranslate           (B,3) the final shifts
    PointcloudScaleAndTranslate   ((B,3) scales, (B,3) shifts)
    PointcloudJitter              (B,N,3) the noise before the clamp
    PointcloudRandomInputDropout  ((B,) the final ratio, (B,N) the per-point uniforms compared with it)
    RandomHorizontalFlip          (B,3) [gate, lower axis, higher axis] uniforms

A contiguous float32 GPU tensor takes the kernel; anything else (CPU, strided, another dtype) takes `augment_torch`, a vectorised
restatement of the same arithmetic with the kernel's own arguments -- the CPU tests' subject and the GPU tests' second opinion.
A launch holds at most MAX_OPS ops, one dropout and one jitter; a longer chain is split into consecutive launches, each with its
own (at most three) draw calls.
"""
import ctypes
import math

import torch

from .engine_pretrain import PointcloudScaleAndTranslate

# the op codes of include/gm3d.h
ROTATE, SCALE, TRANSLATE, SCALE_TRANSLATE, JITTER, DROPOUT, FLIP = 1, 2, 3, 4, 5, 6, 7
FINAL = 0x100
MAX_OPS = 8
GROUPS = {ROTATE: (1,), SCALE: (3,), TRANSLATE: (3,), SCALE_TRANSLATE: (3, 3), JITTER: (), DROPOUT: (1,), FLIP: (3,)}


def _f32(v):
    """the float32 the C ABI receives for the Python float v"""
    return ctypes.c_float(v).value


class _Transform(object):
    def __call__(self, pc, draws=None, generator=None):
        return Compose([self])(pc, draws=None if draws is None else [draws], generator=generator)


class PointcloudRotate(_Transform):
    """P/datasets/data_transforms.py:6-18: a rotation about the y axis by 2 pi u, one u per cloud."""
    kind = ROTATE

    def params(self):
        return (0.0, 0.0, 0.0)


class PointcloudJitter(_Transform):
    """P/:37-49: pc += clamp(N(0, std), -clip, clip), per coordinate."""
    kind = JITTER

    def __init__(self, std=0.01, clip=0.05):
        self.std, self.clip = std, clip

    def params(self):
        return (self.std, self.clip, 0.0)


class PointcloudScale(_Transform):
    """P/:51-63: pc * s, s ~ U[scale_low, scale_high] per cloud and axis."""
    kind = SCALE

    def __init__(self, scale_low=2. / 3., scale_high=3. / 2.):
        self.scale_low, self.scale_high = scale_low, scale_high

    def params(self):
        return (self.scale_low, self.scale_high - self.scale_low, 0.0)


class PointcloudTranslate(_Transform):
    """P/:65-76: pc + t, t ~ U[-translate_range, translate_range] per cloud and axis."""
    kind = TRANSLATE

    def __init__(self, translate_range=0.2):
        self.translate_range = translate_range

    def params(self):
        return (self.translate_range, 0.0, 0.0)


class PointcloudRandomInputDropout(_Transform):
    """P/:79-94: ratio = u * max_dropout_ratio per cloud; every point whose own uniform is <= ratio becomes the cloud's point 0."""
    kind = DROPOUT

    def __init__(self, max_dropout_ratio=0.5):
        assert max_dropout_ratio >= 0 and max_dropout_ratio < 1
        self.max_dropout_ratio = max_dropout_ratio

    def params(self):
        return (self.max_dropout_ratio, 0.0, 0.0)


class RandomHorizontalFlip(_Transform):
    """P/:96-118: with probability 0.95, each of the two axes that are not upright is mirrored (max - coordinate) with
    probability 0.5.  The 4-D temporal form is not built."""
    kind = FLIP

    def __init__(self, upright_axis='z', is_temporal=False):
        if is_temporal:
            raise NotImplementedError("RandomHorizontalFlip(is_temporal=True): clouds here are (B,N,3)")
        self.is_temporal = False
        self.D = 3
        self.upright_axis = {'x': 0, 'y': 1, 'z': 2}[upright_axis.lower()]
        self.horz_axes = set(range(self.D)) - set([self.upright_axis])

    def params(self):
        return (float(self.upright_axis), 0.0, 0.0)


def _spec(t):
    """transform -> (op code, its three parameters as the float32 values the kernel receives)"""
    if isinstance(t, PointcloudScaleAndTranslate):
        kind, p = SCALE_TRANSLATE, (t.scale_low, t.scale_high - t.scale_low, t.translate_range)
    elif isinstance(t, _Transform):
        kind, p = t.kind, t.params()
    else:
        raise TypeError("Compose takes the transforms of gm3d_amd.data_transforms, not %r" % (t,))
    return kind, tuple(_f32(v) for v in p)


class Program(object):
    """What one gm3d_augment launch receives from the host: codes (op | FINAL), params (three floats per op), cols (each op's first
    column in cloud_u, the running sum of the draw counts) and D (their total)."""

    def __init__(self, transforms, final=None):
        if not 1 <= len(transforms) <= MAX_OPS:
            raise ValueError("a launch holds 1..%d ops, not %d" % (MAX_OPS, len(transforms)))
        final = final if final is not None else [False] * len(transforms)
        self.codes, self.params, self.cols, self.D = [], [], [], 0
        for t, f in zip(transforms, final):
            kind, p = _spec(t)
            self.codes.append(kind | (FINAL if f and kind not in (ROTATE, FLIP) else 0))
            self.params.append(p)
            self.cols.append(self.D)
            self.D += sum(GROUPS[kind])
        kinds = [c & 0xff for c in self.codes]
        if kinds.count(DROPOUT) > 1 or kinds.count(JITTER) > 1:
            raise ValueError("a launch holds at most one dropout and one jitter")

    def __len__(self):
        return len(self.codes)


def split(transforms):
    """[(start, end)]: the consecutive launches of a chain -- at most MAX_OPS ops, one dropout and one jitter each."""
    out, start, seen = [], 0, set()
    for i, t in enumerate(transforms):
        kind = _spec(t)[0]
        if i - start == MAX_OPS or (kind in (DROPOUT, JITTER) and kind in seen):
            out.append((start, i))
            start, seen = i, set()
        seen.add(kind)
    if start < len(transforms):
        out.append((start, len(transforms)))
    return out


def _group(cloud_u, B, col, cnt):
    """the (B,cnt) block of the draw group that starts at column col (include/gm3d.h: one block per group, in column order)"""
    return cloud_u[B * col:B * (col + cnt)].view(B, cnt)


def augment_torch(pc, prog, cloud_u, point_u=None, point_z=None):
    """gm3d_augment restated with torch ops, argument for argument: pc (B,N,3) float32 (any device, any strides) is modified in
    place.  Every product and sum is its own float32 op; angles and thresholds are float64, like the kernel's."""
    B = pc.shape[0]
    x, y, z = pc[..., 0].clone(), pc[..., 1].clone(), pc[..., 2].clone()
    for code, p, col in zip(prog.codes, prog.params, prog.cols):
        kind, fin = code & 0xff, bool(code & FINAL)
        if kind == ROTATE:
            ang = _group(cloud_u, B, col, 1).double() * 2.0 * math.pi
            c, s = torch.cos(ang).float(), torch.sin(ang).float()
            x, z = x * c - z * s, x * s + z * c
        if kind in (SCALE, SCALE_TRANSLATE):
            u = _group(cloud_u, B, col, 3)
            sc = u if fin else u * p[1] + p[0]
            x, y, z = x * sc[:, 0:1], y * sc[:, 1:2], z * sc[:, 2:3]
        if kind in (TRANSLATE, SCALE_TRANSLATE):
            u = _group(cloud_u, B, col + (3 if kind == SCALE_TRANSLATE else 0), 3)
            sh = u if fin else (u * 2 - 1) * (p[2] if kind == SCALE_TRANSLATE else p[0])
            x, y, z = x + sh[:, 0:1], y + sh[:, 1:2], z + sh[:, 2:3]
        if kind == JITTER:
            n = (point_z if fin else point_z * p[0]).clamp(-p[1], p[1])
            x, y, z = x + n[..., 0], y + n[..., 1], z + n[..., 2]
        if kind == DROPOUT:
            u = _group(cloud_u, B, col, 1).double()
            drop = point_u.double() <= (u if fin else u * p[0])
            x, y, z = (torch.where(drop, v[:, 0:1], v) for v in (x, y, z))
        if kind == FLIP:
            u = _group(cloud_u, B, col, 3).double()
            v = [x, y, z]
            for m, ax in enumerate(a for a in range(3) if a != int(p[0])):
                do = (u[:, 0:1] < 0.95) & (u[:, m + 1:m + 2] < 0.5)
                v[ax] = torch.where(do, v[ax].max(dim=1, keepdim=True).values - v[ax], v[ax])
            x, y, z = v
    pc.copy_(torch.stack((x, y, z), dim=-1))
    return pc


class Compose(object):
    """An ordered chain of this module's transforms as one launch per MAX_OPS ops (module docstring)."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        self.launches = split(self.transforms)          # validates the chain as well

    def draw(self, prog, B, N, device, draws, generator):
        """-> (cloud_u (B*D) | None, point_u (B,N) | None, point_z (B,N,3) | None) of one launch: at most three draw calls on
        `generator`, then the injected quantities written over their groups."""
        kinds = [c & 0xff for c in prog.codes]
        f32 = dict(device=device, dtype=torch.float32)
        live = [d is None for d in draws]
        cloud_u = point_u = point_z = None
        if prog.D:
            if any(l and GROUPS[k] for l, k in zip(live, kinds)):
                cloud_u = torch.rand(B, prog.D, generator=generator, **f32).view(-1)
            else:
                cloud_u = torch.zeros(B * prog.D, **f32)
        if DROPOUT in kinds:
            d = draws[kinds.index(DROPOUT)]
            point_u = torch.rand(B, N, generator=generator, **f32) if d is None else d[1].to(**f32).reshape(B, N).contiguous()
        if JITTER in kinds:
            d = draws[kinds.index(JITTER)]
            point_z = torch.randn(B, N, 3, generator=generator, **f32) if d is None else d.to(**f32).reshape(B, N, 3).contiguous()
        for k, col, d in zip(kinds, prog.cols, draws):
            if d is None or k == JITTER:
                continue
            parts = d if k == SCALE_TRANSLATE else (d[0],) if k == DROPOUT else (d,)
            for cnt, part in zip(GROUPS[k], parts):
                _group(cloud_u, B, col, cnt).copy_(torch.as_tensor(part).to(**f32).reshape(B, cnt))
                col += cnt
        return cloud_u, point_u, point_z

    def __call__(self, pc, draws=None, generator=None):
        if pc.dim() != 3 or pc.size(2) != 3:
            raise ValueError("pc must be (B,N,3), got %s" % (tuple(pc.shape),))
        draws = list(draws) if draws is not None else [None] * len(self.transforms)
        if len(draws) != len(self.transforms):
            raise ValueError("draws must hold one entry (or None) per transform: %d for %d" % (len(draws), len(self.transforms)))
        B, N = pc.shape[0], pc.shape[1]
        if B == 0 or N == 0:
            return pc
        kernel = pc.is_cuda and pc.dtype == torch.float32 and pc.is_contiguous()
        for a, b in self.launches:
            prog = Program(self.transforms[a:b], [d is not None for d in draws[a:b]])
            cloud_u, point_u, point_z = self.draw(prog, B, N, pc.device, draws[a:b], generator)
            if kernel:
                from ._capi import lib
                from .ops import _launch, _ptr, _stream
                n = len(prog)
                ops = (ctypes.c_int * n)(*prog.codes)
                params = (ctypes.c_float * (3 * n))(*[v for p in prog.params for v in p])
                _launch("gm3d_augment", {"B": B, "N": N, "nops": n}, lib.gm3d_augment, _ptr(pc), B, N, n, ops, params, _ptr(cloud_u),
                        _ptr(point_u), _ptr(point_z), _stream())
            elif pc.dtype == torch.float32:
                augment_torch(pc, prog, cloud_u, point_u, point_z)
            else:
                pc.copy_(augment_torch(pc.float(), prog, cloud_u, point_u, point_z))
        return pc

"""Generates tests/golden/data_transforms.npz from the reference's own Point-MAE_SA3D/datasets/data_transforms.py: the module is
imported in place (never copied) and its classes run on the CPU, cloud by cloud, exactly as its engines call them.

How the reference is driven
  * Its draws come from np.random.uniform, np.random.random and random.random.  For the run these three names are pointed at a
    recording source whose values are float32-representable (a uniform u is drawn in float32; uniform(low, high) returns
    float32(low + (high - low) u), what the reference's `.float()` would make of it anyway), so the float32 kernel and the float64
    reference decide every threshold on the same number.  What the source handed out is stored as the op's draws.
  * The jitter fills `pc.new(N, 3).normal_(0, std)` from torch's global generator: torch.manual_seed is set in front of the op, and
    the same tensors are drawn again from the same seed and stored (the noise BEFORE the clamp).
  * Scale, Translate and ScaleAndTranslate call `.cuda()` on their draws; inside this script only, Tensor.cuda is the identity.

Stored per N in (1, 33, 1000), B = 4 clouds each (cloud 1 offset by 5 units, cloud 2 scaled to 1e-3), under "n<N>/":
  pc                                  (B,N,3) f32   the input
  rotate/u, rotate/out                (B,), (B,N,3)
  scale/scale, scale/out              (B,3), (B,N,3)           the final scales
  translate/shift, translate/out
  scale_translate/scale, /shift, /out
  jitter/noise, jitter/out            (B,N,3) before the clamp; every jitter here is PointcloudJitter(std=0.01, clip=0.02), stored
                                      as jitter_std_clip at the top level, so that the clamp bites; all other ops have the defaults
  dropout/u, /ratio, /point_u, /out   (B,), (B,), (B,N)        ratio = u * max_dropout_ratio
  flip/u, flip/out                    (B,3) [gate, lower axis, higher axis], 1.0 where the reference drew none
  chainA/...  Scale -> Translate -> Jitter -> RandomInputDropout -> RandomHorizontalFlip: the same keys per op, and chainA/out
  chainB/...  RandomHorizontalFlip -> RandomInputDropout -> ScaleAndTranslate -> Jitter -> Rotate, and chainB/out

Self-check: gm3d_amd.data_transforms' torch restatement, fed the stored draws, reproduces every output -- bit for bit except where
a rotation is involved, there within 2^-21 of the cloud's largest |coordinate| (tests/test_data_transforms_cpu.py derives the bar).

Usage:  python tests/golden/make_golden_data_transforms.py <path of the reference's Point-MAE_SA3D directory>
"""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SIZES = (1, 33, 1000)
B = 4
OPS = ("rotate", "scale", "translate", "scale_translate", "jitter", "dropout", "flip")
CHAINS = {"chainA": ("scale", "translate", "jitter", "dropout", "flip"),
          "chainB": ("flip", "dropout", "scale_translate", "jitter", "rotate")}
JITTER = dict(std=0.01, clip=0.02)           # the reference's default clip (5 std) never bites in 12000 samples: 2 std does


class Source:
    """Stands in for np.random.uniform / np.random.random / random.random; float32-representable values, all recorded."""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.log = []

    def _u(self, size):
        return np.asarray(self.rng.random_sample(size)).astype(np.float32).astype(np.float64)

    def uniform(self, low=0.0, high=1.0, size=None):
        v = np.asarray(low + (high - low) * self._u(size)).astype(np.float32).astype(np.float64)
        self.log.append(v)
        return v if size is not None else float(v)

    def random(self, size=None):
        v = self._u(size)
        self.log.append(np.asarray(v))
        return v if size is not None else float(v)

    def take(self):
        out, self.log = self.log, []
        return out


class patched:
    """the three draw functions -> `src`, Tensor.cuda -> identity, for the block"""

    def __init__(self, src):
        self.src = src

    def __enter__(self):
        self.saved = (np.random.uniform, np.random.random, random.random, torch.Tensor.cuda)
        np.random.uniform, np.random.random, random.random = self.src.uniform, self.src.random, self.src.random
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        np.random.uniform, np.random.random, random.random, torch.Tensor.cuda = self.saved
        return False


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_data_transforms", os.path.join(root, "datasets", "data_transforms.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def make_clouds(N, seed):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (B, N, 3)) * np.array([1.0, 0.6, 0.3])
    x[1] += 5.0
    x[2] *= 1e-3
    return x.astype(np.float32)


def run_op(ref, name, pc, src, seed):
    """runs the reference's op `name` on pc (a torch tensor, modified in place) -> {key: array} of its draws"""
    t = {"rotate": ref.PointcloudRotate, "scale": ref.PointcloudScale, "translate": ref.PointcloudTranslate,
         "scale_translate": ref.PointcloudScaleAndTranslate, "jitter": ref.PointcloudJitter,
         "dropout": ref.PointcloudRandomInputDropout, "flip": ref.RandomHorizontalFlip}[name](**(JITTER if name == "jitter" else {}))
    N = pc.shape[1]
    torch.manual_seed(seed)
    if name == "flip":
        # random.random is called 1 to 3 times per cloud: record cloud by cloud
        u = np.ones((B, 3))
        for i in range(B):
            with patched(src):
                t(pc[i:i + 1])
            got = src.take()
            u[i, :len(got)] = got
        return {"u": u.astype(np.float32)}
    with patched(src):
        t(pc)
    log = src.take()
    if name == "rotate":
        return {"u": np.array(log, dtype=np.float32)}
    if name == "scale":
        return {"scale": np.stack(log).astype(np.float32)}
    if name == "translate":
        return {"shift": np.stack(log).astype(np.float32)}
    if name == "scale_translate":
        return {"scale": np.stack(log[0::2]).astype(np.float32), "shift": np.stack(log[1::2]).astype(np.float32)}
    if name == "dropout":
        u = np.array([float(v) for v in log[0::2]])
        return {"u": u.astype(np.float32), "ratio": (u * t.max_dropout_ratio).astype(np.float32),
                "point_u": np.stack(log[1::2]).astype(np.float32)}
    assert name == "jitter" and not log
    torch.manual_seed(seed)                                   # the same tensors again, before the clamp
    return {"noise": np.stack([pc.new(N, 3).normal_(mean=0.0, std=t.std).numpy() for _ in range(B)])}


def draws_of(name, d):
    """stored draws of one op -> the `draws=` entry of gm3d_amd.data_transforms"""
    g = lambda k: torch.from_numpy(d[k])
    return {"rotate": lambda: g("u"), "scale": lambda: g("scale"), "translate": lambda: g("shift"),
            "scale_translate": lambda: (g("scale"), g("shift")), "jitter": lambda: g("noise"),
            "dropout": lambda: (g("ratio"), g("point_u")), "flip": lambda: g("u")}[name]()


def ours(name):
    from gm3d_amd import data_transforms as T
    return {"rotate": T.PointcloudRotate, "scale": T.PointcloudScale, "translate": T.PointcloudTranslate,
            "scale_translate": T.PointcloudScaleAndTranslate, "jitter": T.PointcloudJitter,
            "dropout": T.PointcloudRandomInputDropout, "flip": T.RandomHorizontalFlip}[name](**(JITTER if name == "jitter" else {}))


def self_check(names, pc, draws, want):
    from gm3d_amd import data_transforms as T
    got = T.Compose([ours(n) for n in names])(torch.from_numpy(pc.copy()), draws=[draws_of(n, d) for n, d in zip(names, draws)]).numpy()
    if "rotate" not in names:
        assert np.array_equal(got, want), names
        return 0.0
    err = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)
    assert err.max() <= 2.0 ** -21, (names, err)
    return err.max()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    out, worst = {"jitter_std_clip": np.array([JITTER["std"], JITTER["clip"]])}, 0.0
    for N in SIZES:
        pc = make_clouds(N, 100 + N)
        out["n%d/pc" % N] = pc
        for k, name in enumerate(OPS):
            x = torch.from_numpy(pc.copy())
            d = run_op(ref, name, x, Source(1000 * N + k), seed=7 * N + k)
            assert x.dtype == torch.float32
            for key, v in d.items():
                out["n%d/%s/%s" % (N, name, key)] = v
            out["n%d/%s/out" % (N, name)] = x.numpy()
            worst = max(worst, self_check([name], pc, [d], x.numpy()))
        for c, (chain, names) in enumerate(CHAINS.items()):
            x = torch.from_numpy(pc.copy())
            src, ds = Source(5000 * N + c), []
            for k, name in enumerate(names):
                ds.append(run_op(ref, name, x, src, seed=11 * N + 3 * c + k))
                for key, v in ds[-1].items():
                    out["n%d/%s/%s/%s" % (N, chain, name, key)] = v
            out["n%d/%s/out" % (N, chain)] = x.numpy()
            worst = max(worst, self_check(names, pc, ds, x.numpy()))
    path = os.path.join(HERE, "data_transforms.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; largest rotation error %.2e of the cloud's largest coordinate (bar %.2e)"
          % (path, len(out), os.path.getsize(path), worst, 2.0 ** -21))


if __name__ == "__main__":
    main()

"""Generates tests/golden/shapenet_dataset.npz from the reference's own per-sample data path: `ShapeNet.random_sample` and
`ShapeNet.pc_norm` of /root/reference/Point-MAE_SA3D/datasets/ShapeNet55Dataset.py:45-57 (plain NumPy; the module is imported in
place, never copied).  This is what gm3d_sample_normalize (gm3d_amd/csrc/dataset.hip) replaces.

How the reference is driven: a `ShapeNet` instance is made WITHOUT its __init__ (which reads the dataset's file lists), its
`permutation` is set to arange(N_POINTS) as __init__ does (:44), NumPy is seeded, and per cloud `random_sample(cloud, num)` then
`pc_norm(...)` run exactly as __getitem__ runs them (:64-65).  random_sample shuffles the instance's permutation IN PLACE, so the
permutation of cloud i is a shuffle of cloud i-1's: the permutation the reference held after each call is stored, and the test
turns it into keys (keys[perm[j]] = j / N0) that rank the points in that very order.

Stored per case (name/...):
  clouds   (M,N0,3) f32   the raw clouds (the first half centred, the second half offset by 5 units per axis; M = 2 x kind)
  perm     (M,N0)  int16  the permutation the reference drew for each cloud
  num      ()      int64
  out32    (M,num,3) f32  the reference's output on the float32 clouds (np.mean etc. in fp32: what the reference computes)
  out64    (M,num,3) f64  the same pc_norm on the same points as float64
  ref_err  (M,)    f64    max |out32 - out64| per cloud: the reference's own fp32 error, the yardstick of the test's error bar

Usage:  python tests/golden/make_golden_dataset.py        (writes next to this file)
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/Point-MAE_SA3D"
CASES = [  # name, clouds of each kind (centred / offset), N_POINTS, num, seed
    ("n2048_256", 2, 2048, 256, 21),         # 4 clouds
    ("n8192_1024", 1, 8192, 1024, 22),       # ShapeNet55 pre-training: 8192 -> 1024; 1 cloud of each kind
    ("n33_7", 1, 33, 7, 23),                 # 2 clouds
]


def load_reference_dataset():
    """The module's imports that do not bear on the two methods (its IO class, the dataset registry, the logger) are satisfied
    by stand-in modules; the method bodies that run are the reference's own."""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    pkg = mod("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    mod("datasets.build", DATASETS=_Registry())
    mod("datasets.io", IO=object)
    mod("utils")
    mod("utils.logger")
    spec = importlib.util.spec_from_file_location("datasets.ShapeNet55Dataset", os.path.join(REF, "datasets", "ShapeNet55Dataset.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["datasets.ShapeNet55Dataset"] = m
    spec.loader.exec_module(m)
    return m.ShapeNet


def make_clouds(M, N, seed):
    """M clouds of each kind: centred (uniform in a box of uneven sides), and the same family offset by 5 units per axis, where the
    fp32 mean costs the most."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (2 * M, N, 3)) * np.array([1.0, 0.6, 0.3])
    x[M:] += 5.0
    return x.astype(np.float32)


def one_case(ShapeNet, M, N, num, seed):
    clouds = make_clouds(M, N, seed)
    ds = ShapeNet.__new__(ShapeNet)                  # no __init__: no file lists
    ds.npoints, ds.sample_points_num = N, num
    ds.permutation = np.arange(N)                    # ShapeNet55Dataset.py:44
    np.random.seed(seed)
    perms, out32, out64 = [], [], []
    for c in clouds:
        picked = ds.random_sample(c, num)            # shuffles ds.permutation in place, takes [:num]
        perm = ds.permutation.copy()
        assert np.array_equal(picked, c[perm[:num]]) and picked.dtype == np.float32
        o32 = ds.pc_norm(picked)
        assert o32.dtype == np.float32
        o64 = ds.pc_norm(c.astype(np.float64)[perm[:num]])
        perms.append(perm.astype(np.int16))
        out32.append(o32)
        out64.append(o64)
    out32, out64 = np.stack(out32), np.stack(out64)
    err = np.abs(out32.astype(np.float64) - out64).reshape(len(clouds), -1).max(1)
    return clouds, np.stack(perms), out32, out64, err


def main():
    ShapeNet = load_reference_dataset()
    out = {}
    for name, M, N, num, seed in CASES:
        clouds, perm, o32, o64, err = one_case(ShapeNet, M, N, num, seed)
        out[name + "/clouds"], out[name + "/perm"], out[name + "/num"] = clouds, perm, np.int64(num)
        out[name + "/out32"], out[name + "/out64"], out[name + "/ref_err"] = o32, o64, err
        print("%-12s %d clouds  N=%d num=%d  reference fp32 error vs fp64: centred %.2e, offset %.2e"
              % (name, len(clouds), N, num, err[:M].max(), err[M:].max()))
    path = os.path.join(HERE, "shapenet_dataset.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

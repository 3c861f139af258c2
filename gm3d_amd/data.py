"""Device-resident datasets: the whole dataset sits in HBM and every batch is assembled on the GPU by one launch.

The reference feeds its loops from a `DataLoader` over datasets/ShapeNet55Dataset.py (per sample: np.load, an in-place shuffle of an
8192-long permutation, a fancy-index gather, pc_norm; then collate and a host-to-device copy), ModelNetDataset.py and
ScanObjectNNDataset.py (a shuffle of all points on the train split).  Here `DeviceDataset` holds the (M,N0,3) clouds on the device,
and `DeviceLoader` yields batches in the shapes the engines unpack, each one made by `sample_normalize` (gm3d_sample_normalize,
csrc/dataset.hip): pick the batch's clouds, take a random ordered subset of each cloud's points, centre and scale it.

  ds = DeviceDataset.from_arrays(points, npoints=1024, normalize=True)          # ShapeNet55 pre-training
  loader = DeviceLoader(ds, 128, seed=0)
  for epoch in ...:
      loader.set_epoch(epoch)
      engine_pretrain_point_mae.train_one_epoch(model, loader, optimizer, "cuda", epoch, args)

IO is out of scope beyond `np.load`: no h5py, no open3d, no parsers for the datasets' own file formats.
"""
import math

import numpy as np
import torch

from ._capi import lib
from .ops import _launch, _ptr, _require, _stream

MAX_POINTS = 8192          # gm3d_sample_normalize: N0 <= 8192


def sample_normalize(data, cloud_idx, keys, num, normalize, return_idx=False):
    """data (M,N0,3) f32, cloud_idx (B) int64, keys (B,N0) f32, all contiguous on the GPU -> out (B,num,3) f32 [, idx (B,num) int32].
    Row j of cloud b is the point with the j-th smallest (key, index) of keys[b] (-0 == +0, NaN last); normalize: pc_norm of the
    selected points (minus their mean, divided by the largest norm), else bit copies.  One launch."""
    _require(data, torch.float32, "data")
    _require(cloud_idx, torch.int64, "cloud_idx")
    _require(keys, torch.float32, "keys")
    if data.dim() != 3 or data.size(2) != 3:
        raise RuntimeError("data must be (M,N0,3)")
    M, N0, _ = data.shape
    if cloud_idx.dim() != 1 or keys.dim() != 2 or keys.shape != (cloud_idx.shape[0], N0):
        raise RuntimeError("cloud_idx must be (B) and keys (B,N0)")
    if cloud_idx.device != data.device or keys.device != data.device:
        raise RuntimeError("data, cloud_idx and keys must be on the same device")
    B, num = cloud_idx.shape[0], int(num)
    out = torch.empty(B, max(num, 0), 3, dtype=torch.float32, device=data.device)
    idx = torch.empty(B, max(num, 0), dtype=torch.int32, device=data.device) if return_idx else None
    _launch("gm3d_sample_normalize", {"B": B, "N0": N0, "num": num, "normalize": int(bool(normalize))}, lib.gm3d_sample_normalize,
            _ptr(data), _ptr(cloud_idx), _ptr(keys), B, M, N0, num, int(bool(normalize)), _ptr(out), _ptr(idx), _stream())
    return (out, idx) if return_idx else out


class DeviceDataset:
    """(M,N0,3) float32 clouds, moved to the device once, with what a batch is made of:
    npoints         points per yielded cloud (None: all N0 -- the ModelNet / ScanObjectNN form, a permutation of the cloud);
    normalize       pc_norm of the selected points (ShapeNet55Dataset.py:45-51);
    shuffle_points  False: the file's order, its first npoints points (the reference's test splits);
    labels          (M) integer labels: the loader then yields (name, "sample", (points, labels)) like the labelled datasets;
    name            the first element of that tuple."""

    def __init__(self, points, labels=None, npoints=None, normalize=False, shuffle_points=True, device="cuda", name="DeviceDataset"):
        points = torch.as_tensor(points)
        if points.dim() != 3 or points.size(2) != 3 or points.dtype != torch.float32:
            raise RuntimeError("points must be (M,N0,3) float32")
        if points.size(0) < 1 or not 1 <= points.size(1) <= MAX_POINTS:
            raise RuntimeError("points must hold at least one cloud of 1..%d points" % MAX_POINTS)
        self.points = points.to(device).contiguous()
        if not self.points.is_cuda:
            raise RuntimeError("a DeviceDataset lives on a GPU (gm3d_amd has no CPU fallback)")
        self._init(labels, npoints, normalize, shuffle_points, name)

    def _init(self, labels, npoints, normalize, shuffle_points, name):
        M, N0, _ = self.points.shape
        self.npoints = N0 if npoints is None else int(npoints)
        if not 1 <= self.npoints <= N0:
            raise RuntimeError("npoints must be in 1..%d" % N0)
        self.normalize, self.shuffle_points, self.name = bool(normalize), bool(shuffle_points), name
        self.labels = None
        if labels is not None:
            labels = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).reshape(-1)
            if labels.shape[0] != M:
                raise RuntimeError("labels must hold one entry per cloud")
            self.labels = labels.to(self.points.device, torch.int64)

    @classmethod
    def from_arrays(cls, points, labels=None, **kw):
        """In-memory arrays: points (M,N0,3) (cast to float32 like the reference's `.astype(np.float32)`), labels (M) or None."""
        if not isinstance(points, torch.Tensor):
            points = np.ascontiguousarray(points, dtype=np.float32)
        return cls(torch.as_tensor(points).float(), labels, **kw)

    @classmethod
    def from_npy_files(cls, paths, labels=None, npoints=None, normalize=False, shuffle_points=True, device="cuda",
                       name="DeviceDataset"):
        """One (N0,3) `.npy` file per cloud (ShapeNet55's layout), read with np.load one at a time into a device tensor allocated
        once: the host never holds more than one cloud."""
        paths = list(paths)
        if not paths:
            raise RuntimeError("no files")
        first = np.load(paths[0])
        if first.ndim != 2 or first.shape[1] != 3 or not 1 <= first.shape[0] <= MAX_POINTS:
            raise RuntimeError("%s: expected an (N0,3) array with N0 <= %d, got %s" % (paths[0], MAX_POINTS, first.shape))
        self = cls.__new__(cls)
        self.points = torch.empty((len(paths),) + first.shape, dtype=torch.float32, device=device)
        if not self.points.is_cuda:
            raise RuntimeError("a DeviceDataset lives on a GPU (gm3d_amd has no CPU fallback)")
        for i, p in enumerate(paths):
            a = first if i == 0 else np.load(p)
            if a.shape != first.shape:
                raise RuntimeError("%s: shape %s differs from %s" % (p, a.shape, first.shape))
            self.points[i].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        self._init(labels, npoints, normalize, shuffle_points, name)
        return self

    def __len__(self):
        return self.points.shape[0]


def epoch_order(M, epoch, shuffle=True, seed=0, rank=0, world=1):
    """The indices `torch.utils.data.DistributedSampler(range(M), world, rank, shuffle, seed, drop_last=False)` yields after
    set_epoch(epoch), as a list: randperm on a CPU generator seeded seed + epoch (or 0..M-1), padded from its own start to a
    multiple of `world`, then every world-th index from `rank` on."""
    if not 0 <= rank < world:
        raise ValueError("rank must be in 0..world-1")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        order = torch.randperm(M, generator=g).tolist()
    else:
        order = list(range(M))
    total = int(math.ceil(M / world)) * world
    pad = total - M
    if pad <= M:
        order += order[:pad]
    else:
        order += (order * int(math.ceil(pad / M)))[:pad]
    return order[rank:total:world]


class DeviceLoader:
    """Batches of a DeviceDataset in the order of the reference's DistributedSampler + DataLoader, assembled on the device.

    Per epoch: the cloud order is computed on the host (epoch_order) and copied over once.  Per batch: one torch.rand((B,N0)) on
    the loader's own device generator (seeded seed + rank; never the default generator, whose state the captured steps share) and
    one gm3d_sample_normalize launch; shuffle_points=False feeds arange keys instead.  Every batch is a fresh tensor: the engines'
    look-ahead holds two at once.  Without labels a batch is the (B,num,3) tensor, with labels (name, "sample", (points, labels)).
    rank / world default to torch.distributed's when it is initialised, else 0 / 1; `generator` replaces the loader's own."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=True, seed=0, rank=None, world=None, generator=None):
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world = (dist.get_world_size() if on else 1) if world is None else world
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError("batch_size must be >= 1 and rank in 0..world-1")
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.generator, self._own = generator, None
        self.num_samples = int(math.ceil(len(dataset) / self.world))

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self):
        return epoch_order(len(self.dataset), self.epoch, self.shuffle, self.seed, self.rank, self.world)

    def __len__(self):
        return self.num_samples // self.batch_size if self.drop_last else -(-self.num_samples // self.batch_size)

    def _generator(self, device):
        """The loader's own generator is re-seeded from (seed + rank, epoch) when an epoch's iteration starts: the point draws do
        not depend on what was iterated before.  A generator handed in by the caller is used as it is."""
        if self.generator is not None:
            return self.generator
        if self._own is None:
            self._own = torch.Generator(device=device)
        self._own.manual_seed(self.seed + self.rank + 1000003 * self.epoch)
        return self._own

    def __iter__(self):
        ds = self.dataset
        dev = ds.points.device
        N0 = ds.points.shape[1]
        order = torch.tensor(self.order(), dtype=torch.int64).to(dev)          # the epoch's one host-to-device copy
        gen = self._generator(dev) if ds.shuffle_points else None
        fixed = None if ds.shuffle_points else torch.arange(N0, dtype=torch.float32, device=dev)
        for i in range(len(self)):
            idx = order[i * self.batch_size:(i + 1) * self.batch_size]
            B = idx.shape[0]
            if gen is not None:
                keys = torch.rand((B, N0), generator=gen, device=dev, dtype=torch.float32)
            else:
                keys = fixed.expand(B, N0).contiguous()
            pts = sample_normalize(ds.points, idx, keys, ds.npoints, ds.normalize)
            yield pts if ds.labels is None else (ds.name, "sample", (pts, ds.labels[idx]))

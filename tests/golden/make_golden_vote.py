"""Generates tests/golden/vote_b4.npz by running the REFERENCE's own voting evaluation
(/root/reference/Point-MAE_SA3D/tools/runner_finetune.py::test_vote, imported in place, never copied) on CPU in this container,
on the reference's own PointTransformer.  Pins the voting glue: one FPS per batch to point_all, per vote the shared subset
np.random.choice(point_all, npoints, False), the gather, test_transforms (PointcloudScaleAndTranslate, drawn per cloud), the
eval forward, the mean of the votes, argmax and the accuracy arithmetic.

The absent packages are those of make_golden_finetune.install_absent_packages() plus h5py, cv2, timm.scheduler and
torchvision.transforms (Compose = a plain sequential call), stubbed here; torch.Tensor.cuda is the identity.  FPS and gather
come from the CPU oracle.  Weights: oracle.model_ref.det_fill_ (BatchNorm running statistics included), cls_dim 40.
Recorded: the draws themselves (through a recording wrapper of np.random), the per-vote logits (a forward hook), preds, acc and
the fp32 top-2 margin of the vote mean of every cloud.
Usage:  python tests/golden/make_golden_vote.py
"""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/Point-MAE_SA3D"
sys.path.insert(0, ROOT)

from oracle import model_ref as R  # noqa: E402
from tests import clouds  # noqa: E402
from tests.golden import make_golden_finetune as MGF  # noqa: E402

SEED = 2024          # np.random.seed of the run
TIMES = 10
NPOINTS = 1024
BATCHES = ((4, 71), (4, 72), (3, 73))      # (clouds, cloud seed): two full batches of 4 and a ragged batch of 3, 2048 points
LABELS = ((27, 17, 39, 27), (5, 27, 22, 30), (27, 1, 28))   # the fixed weights vote 27 for every cloud: 4 of 11 right


def install_vote_packages():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    mod("h5py")
    mod("cv2")
    mod("timm.scheduler", CosineLRScheduler=object)
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms", Compose=Compose)


class Recorder:
    """Wraps np.random.choice / np.random.uniform (module attributes: the reference calls np.random.<fn> at call time)."""

    def __init__(self):
        self.choice, self.uniform = [], []
        self._c, self._u = np.random.choice, np.random.uniform

    def __enter__(self):
        def choice(*a, **k):
            r = self._c(*a, **k)
            self.choice.append(np.asarray(r).copy())
            return r

        def uniform(*a, **k):
            r = self._u(*a, **k)
            self.uniform.append(np.asarray(r).copy())
            return r

        np.random.choice, np.random.uniform = choice, uniform
        return self

    def __exit__(self, *exc):
        np.random.choice, np.random.uniform = self._c, self._u


def main():
    MGF.install_absent_packages()
    install_vote_packages()
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from models.Point_MAE import PointTransformer  # the reference classes themselves
    from tools import runner_finetune as RF

    cfg = MGF.AttrDict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64,
                       encoder_dims=384)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    ref = PointTransformer(cfg)
    R.det_fill_(ref, seed=5)
    out = {}
    loader = []
    for i, ((B, seed), lab) in enumerate(zip(BATCHES, LABELS)):
        pts = clouds.FAMILIES["gaussian"](B, 2048, seed=seed)
        loader.append((None, None, (pts, torch.tensor(lab))))
        out["pts%d" % i], out["labels%d" % i] = pts.numpy().copy(), np.asarray(lab, dtype=np.int64)

    logits = []
    hook = ref.register_forward_hook(lambda m, inp, o: logits.append(o.detach().clone()))
    np.random.seed(SEED)
    with Recorder() as rec:
        acc = RF.test_vote(ref, loader, 1, None, SimpleNamespace(distributed=False), MGF.AttrDict(npoints=NPOINTS), times=TIMES)
    hook.remove()
    assert len(logits) == TIMES * len(BATCHES) and len(rec.choice) == TIMES * len(BATCHES)
    assert len(rec.uniform) == 2 * TIMES * sum(B for B, _ in BATCHES)

    u = iter(rec.uniform)
    preds, margins = [], []
    for i, (B, _) in enumerate(BATCHES):
        votes = torch.stack(logits[i * TIMES:(i + 1) * TIMES])                 # (V,B,cls)
        out["votes%d" % i] = votes.numpy().copy()
        out["subsets%d" % i] = np.stack(rec.choice[i * TIMES:(i + 1) * TIMES]).astype(np.int64)
        xyz = np.array([[next(u), next(u)] for _ in range(TIMES * B)]).reshape(TIMES, B, 2, 3)
        out["xyz1_%d" % i], out["xyz2_%d" % i] = xyz[:, :, 0].copy(), xyz[:, :, 1].copy()     # float64, as drawn
        mean = votes.mean(0)
        preds.append(mean.argmax(-1))
        top2 = mean.topk(2, dim=-1).values
        margins.append(top2[:, 0] - top2[:, 1])
    out["pred"] = torch.cat(preds).numpy().astype(np.int64)
    out["margin"] = torch.cat(margins).numpy().copy()
    out["acc"] = np.asarray(float(acc), dtype=np.float32)
    out["seed"], out["times"], out["npoints"] = np.int64(SEED), np.int64(TIMES), np.int64(NPOINTS)
    labels = np.concatenate([out["labels%d" % i] for i in range(len(BATCHES))])
    assert float(acc) == float(torch.tensor(int((out["pred"] == labels).sum())) / float(labels.size) * 100.)
    np.savez_compressed(os.path.join(HERE, "vote_b4.npz"), **out)
    print("wrote vote_b4.npz: acc %.4f, min margin %.3g" % (float(acc), float(out["margin"].min())),
          {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()

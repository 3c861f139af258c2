"""Generates tests/golden/reconstruct.npz by running the REFERENCE's own Point_MAE.forward(..., vis=True)
(Point-MAE_SA3D/models/Point_MAE.py:428-439, imported in place, never copied) on the CPU, through the stand-ins
make_golden_published.install() provides for the absent third-party packages -- exactly like make_golden_point_mae.py: the model
section of cfgs/config.yaml (mask ratio 0.6, 64 groups of 32), det_fill_(seed=41), eval mode, gaussian clouds of 1024 points.

Cases: rand + cdl2 at B = 1, rand + cdl2 at B = 2, block + cdl2 at B = 2 (the tie-gap rule of make_golden_point_mae.py: every cloud's
sorted centre distances keep a smallest gap above 1e-6, else the next seed).  The B = 1 cloud is the first of the B = 2 clouds.
Per case: the mask the reference drew (through the same MAE_encoder.forward spy), ret2 (the visible part), `rebuilt` (the rows of ret1
behind ret2: ret1 == [ret2 | rebuilt] is asserted here and the head is stored once), full_center, the loss of a second call with
vis=False under the same seeds, and ac_err: the relative error (largest error over largest entry) of the rebuilt rows when the
reference itself runs under torch.autocast("cpu", torch.bfloat16) -- the yardstick of the bf16 test.

Usage:  python tests/golden/make_golden_reconstruct.py
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import model_ref as R  # noqa: E402
from oracle import ops as O  # noqa: E402
from tests import clouds  # noqa: E402
from tests.golden import make_golden_published  # noqa: E402
from tests.golden.make_golden_finetune import AttrDict, npy  # noqa: E402
from tests.golden.make_golden_point_mae import REF, min_gap  # noqa: E402

CASES = (("rand_b1", "rand", 1), ("rand_b2", "rand", 2), ("block_b2", "block", 2))


def seeded(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(5)


def main():
    make_golden_published.install()
    sys.path.insert(0, REF)
    from models.Point_MAE import Point_MAE

    base = json.load(open(os.path.join(REF, "cfgs", "config.yaml")))["model"]
    all_pts = clouds.FAMILIES["gaussian"](2, 1024, seed=2468)
    out = {"pts": npy(all_pts)}
    for ci, (name, mask_type, B) in enumerate(CASES):
        pts = all_pts[:B]
        cfg = AttrDict({**base, "loss": "cdl2", "transformer_config": AttrDict({**base["transformer_config"], "mask_type": mask_type})})
        torch.manual_seed(0)
        model = Point_MAE(cfg)
        model.loss_func = O.ChamferDistanceL2(reduction="mean")
        R.det_fill_(model, seed=41)
        model.eval()
        seed = 300 + ci
        if mask_type == "block":
            with torch.no_grad():
                center = model.group_divider(pts.clone())[1]
            while True:
                random.seed(seed)
                start = [random.randint(0, center.shape[1] - 1) for _ in range(B)]
                if min_gap(center, start) > 1e-6:
                    break
                seed += 1
            out[name + "/start"] = np.array(start, dtype=np.int32)
        out[name + "/seed"] = np.array(seed)
        masks = []
        enc_forward = model.MAE_encoder.forward

        def spy(*a, **k):
            x, m = enc_forward(*a, **k)
            masks.append(m)
            return x, m
        model.MAE_encoder.forward = spy
        with torch.no_grad():
            seeded(seed)
            ret1, ret2, full_center = model(pts.clone(), vis=True)
            seeded(seed)
            loss = model(pts.clone())
            seeded(seed)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                ac1, _, _ = model(pts.clone(), vis=True)
        model.MAE_encoder.forward = enc_forward
        assert len(masks) == 3 and torch.equal(masks[0], masks[1]) and torch.equal(masks[0], masks[2])
        M = int(masks[0][0].sum())
        G, k = masks[0].shape[1], ret1.shape[1] // (B * masks[0].shape[1])
        assert int(masks[0].sum(1).min()) == int(masks[0].sum(1).max()) == M == int(0.6 * G)
        nv = B * (G - M) * k
        assert tuple(ret1.shape) == (1, B * G * k, 3) and tuple(ret2.shape) == (1, nv, 3) and tuple(full_center.shape) == (B * G, 3)
        assert torch.equal(ret1[:, :nv], ret2)
        rebuilt, ac = ret1[0, nv:].float(), ac1[0, nv:].float()
        ac_err = float((ac - rebuilt).abs().max() / rebuilt.abs().max())
        assert torch.equal(ac1[0, :nv].float(), ret2[0])          # autocast does not touch the visible rows
        out[name + "/mask"] = npy(masks[0])
        out[name + "/ret2"] = npy(ret2[0])
        out[name + "/rebuilt"] = npy(rebuilt)
        out[name + "/full_center"] = npy(full_center)
        out[name + "/loss"] = npy(loss)
        out[name + "/ac_err"] = np.array(ac_err)
        print(name, "seed", seed, "shapes", tuple(ret1.shape), tuple(ret2.shape), tuple(full_center.shape), "loss", float(loss),
              "ac_err", ac_err)
    path = os.path.join(HERE, "reconstruct.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Generates tests/golden/point_mae_pretrain_groups.npz by running the REFERENCE's own plain Point-MAE pre-training model
(/root/reference/Point-MAE_SA3D/models/Point_MAE.py::Point_MAE, imported in place, never copied) at its two other pre-training
geometries, on the CPU, through the stand-ins make_golden_published.install() provides (see make_golden_point_mae.py):

    g128k16_cdl2   the model section of config_2.yaml: 128 groups x 16 points, mask ratio 0.75, cdl2
    g256k8_cdl2    the model section of config_3.yaml: 256 groups x 8 points, mask ratio 0.6, cdl2
    g256k8_cdl1    the same with loss = cdl1

B = 4 gaussian clouds of 1024 points, train mode, det_fill_ weights.  Per case: the clouds, the mask the reference drew (np.random),
the DropPath draws, the loss, and the gradients of the six parameters of point_mae_pretrain_b4.npz (tensors above 20000 elements:
every 31st element, plus the norm of the whole).  Each case also records num_group, group_size and mask_ratio as the config gave them.

Usage:  python tests/golden/make_golden_point_mae_groups.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/Point-MAE_SA3D"
sys.path.insert(0, ROOT)

from oracle import model_ref as R  # noqa: E402
from oracle import ops as O  # noqa: E402
from tests import clouds  # noqa: E402
from tests.golden import make_golden_published  # noqa: E402
from tests.golden.make_golden_finetune import AttrDict, npy  # noqa: E402
from tests.golden.make_golden_point_mae import GRADS, STRIDE, picked  # noqa: E402

CASES = (("g128k16_cdl2", "config_2.yaml", "cdl2"), ("g256k8_cdl2", "config_3.yaml", "cdl2"), ("g256k8_cdl1", "config_3.yaml", "cdl1"))


def main():
    make_golden_published.install()
    sys.path.insert(0, REF)
    from models.Point_MAE import Point_MAE

    B = 4
    pts = clouds.FAMILIES["gaussian"](B, 1024, seed=2468)
    out = {"pts": npy(pts), "stride": np.array(STRIDE)}
    for ci, (name, cfg_file, loss) in enumerate(CASES):
        base = json.load(open(os.path.join(REF, cfg_file)))["model"]
        cfg = AttrDict({**base, "loss": loss, "transformer_config": AttrDict(base["transformer_config"])})
        torch.manual_seed(0)
        model = Point_MAE(cfg)
        if loss == "cdl2":
            model.loss_func = O.ChamferDistanceL2(reduction="mean")
        R.det_fill_(model, seed=41)
        model.train()
        seed = 200 + ci
        np.random.seed(seed)
        out[name + "/seed"] = np.array(seed)
        G, k, ratio = base["num_group"], base["group_size"], base["transformer_config"]["mask_ratio"]
        out[name + "/num_group"], out[name + "/group_size"], out[name + "/mask_ratio"] = np.array(G), np.array(k), np.array(ratio)
        R._droppath_log = []
        torch.manual_seed(5)
        masks = []
        enc_forward = model.MAE_encoder.forward

        def spy(*a, **kw):
            x, m = enc_forward(*a, **kw)
            masks.append(m)
            return x, m
        model.MAE_encoder.forward = spy
        lossv = model(pts.clone())
        model.MAE_encoder.forward = enc_forward
        out[name + "/droppath_masks"] = npy(torch.stack(R._droppath_log))
        R._droppath_log = None
        out[name + "/mask"] = npy(masks[0])
        assert tuple(masks[0].shape) == (B, G)
        assert int(masks[0].sum(1).min()) == int(masks[0].sum(1).max()) == int(ratio * G)
        out[name + "/loss"] = npy(lossv)
        lossv.backward()
        named = dict(model.named_parameters())
        assert tuple(named["increase_dim.0.weight"].shape) == (3 * k, 384, 1)
        for key in GRADS:
            g = named[key].grad
            out[name + "/gradnorm/" + key] = npy(g.double().norm())
            out[name + "/grad/" + key] = npy(picked(g))
        print(name, "seed", seed, "loss", float(lossv), "masked", int(masks[0][0].sum()), "of", G)
    path = os.path.join(HERE, "point_mae_pretrain_groups.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""Generates tests/golden/point_mae_pretrain_b4.npz by running the REFERENCE's own plain Point-MAE pre-training model
(/root/reference/Point-MAE_SA3D/models/Point_MAE.py::Point_MAE, imported in place, never copied) with the model section of
cfgs/config.yaml (mask ratio 0.6) on the CPU, through the stand-ins make_golden_published.install() provides for the absent
third-party packages (oracle-backed FPS / KNN / Chamfer: "parity unpinned"; timm Block / DropPath from the oracle's restatement).

Cases: rand + cdl2, rand + cdl1, block + cdl2 on B = 4 gaussian clouds of 1024 points, train mode, det_fill_ weights.  Per case: the
mask the reference drew (np.random for rand, Python's random for block: the drawn start indices are recorded), the DropPath draws,
the loss, and the gradients of six parameters (tensors above 20000 elements: every 31st element, plus the norm of the whole).
`extensions.chamfer_dist.ChamferDistanceL2()` of the reference is the scalar mean(d1) + mean(d2); the oracle's class needs
reduction="mean" for that, which is set on the model after construction.

block: every cloud's sorted centre distances must have a smallest gap above 1e-6 (no argsort ties can enter the fixture); the
generator moves to the next seed otherwise.

Usage:  python tests/golden/make_golden_point_mae.py
"""
import json
import os
import random
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

GRADS = ("mask_token", "increase_dim.0.weight", "MAE_encoder.encoder.first_conv.0.weight", "MAE_encoder.blocks.blocks.0.attn.qkv.weight",
         "MAE_decoder.blocks.0.mlp.fc1.weight", "decoder_pos_embed.0.weight")
CASES = (("rand_cdl2", "rand", "cdl2"), ("rand_cdl1", "rand", "cdl1"), ("block_cdl2", "block", "cdl2"))
STRIDE = 31


def picked(g):
    return g if g.numel() <= 20000 else g.flatten()[::STRIDE]


def min_gap(center, start):
    """smallest gap between consecutive sorted distances to the start centre, per cloud (as _mask_center_block measures them)."""
    gaps = []
    for pts, i in zip(center, start):
        d = torch.norm(pts[i].reshape(1, 3) - pts, p=2, dim=-1)
        gaps.append(float(torch.sort(d)[0].diff().min()))
    return min(gaps)


def main():
    make_golden_published.install()
    sys.path.insert(0, REF)
    from models.Point_MAE import Point_MAE

    base = json.load(open(os.path.join(REF, "cfgs", "config.yaml")))["model"]
    B = 4
    pts = clouds.FAMILIES["gaussian"](B, 1024, seed=1357)
    out = {"pts": npy(pts), "stride": np.array(STRIDE)}
    for ci, (name, mask_type, loss) in enumerate(CASES):
        cfg = AttrDict({**base, "loss": loss, "transformer_config": AttrDict({**base["transformer_config"], "mask_type": mask_type})})
        torch.manual_seed(0)
        model = Point_MAE(cfg)
        if loss == "cdl2":
            model.loss_func = O.ChamferDistanceL2(reduction="mean")
        R.det_fill_(model, seed=41)
        model.train()
        seed = 100 + ci
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
            out[name + "/center"] = npy(center)
            random.seed(seed)
        np.random.seed(seed)
        out[name + "/seed"] = np.array(seed)
        R._droppath_log = []
        torch.manual_seed(5)
        # the reference's forward (P/:400-441), with the mask kept: forward() itself does not return it
        masks = []
        enc_forward = model.MAE_encoder.forward

        def spy(*a, **k):
            x, m = enc_forward(*a, **k)
            masks.append(m)
            return x, m
        model.MAE_encoder.forward = spy
        lossv = model(pts.clone())
        model.MAE_encoder.forward = enc_forward
        out[name + "/droppath_masks"] = npy(torch.stack(R._droppath_log))
        R._droppath_log = None
        out[name + "/mask"] = npy(masks[0])
        assert int(masks[0].sum(1).min()) == int(masks[0].sum(1).max()) == int(0.6 * 64)
        out[name + "/loss"] = npy(lossv)
        lossv.backward()
        named = dict(model.named_parameters())
        for k in GRADS:
            g = named[k].grad
            out[name + "/gradnorm/" + k] = npy(g.double().norm())
            out[name + "/grad/" + k] = npy(picked(g))
        print(name, "seed", seed, "loss", float(lossv), "masked", int(masks[0][0].sum()))
    path = os.path.join(HERE, "point_mae_pretrain_b4.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

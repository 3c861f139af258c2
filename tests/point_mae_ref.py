"""Plain-PyTorch restatement of the reference's Point-MAE pre-training forward (Point-MAE_SA3D/models/Point_MAE.py:322-343,400-441)
on the CPU oracle's operators and modules.  Test infrastructure only: tests/golden/point_mae_pretrain_b4.npz (made by the
reference's own model file) pins it, and the GPU tests may then lean on it where the fixture has no case."""
import torch

from oracle import model_ref as R
from oracle import ops as O
from oracle.published_ref import FrozenPointMAE

CFG = {"group_size": 32, "num_group": 64, "loss": "cdl2",
       "transformer_config": {"mask_ratio": 0.6, "mask_type": "rand", "trans_dim": 384, "encoder_dims": 384, "depth": 12,
                              "drop_path_rate": 0.1, "num_heads": 6, "decoder_depth": 4, "decoder_num_heads": 6}}
GRADS = ("mask_token", "increase_dim.0.weight", "MAE_encoder.encoder.first_conv.0.weight", "MAE_encoder.blocks.blocks.0.attn.qkv.weight",
         "MAE_decoder.blocks.0.mlp.fc1.weight", "decoder_pos_embed.0.weight")
CASES = (("rand_cdl2", "rand", "cdl2"), ("rand_cdl1", "rand", "cdl1"), ("block_cdl2", "block", "cdl2"))


def config(mask_type="rand", loss="cdl2", **kw):
    cfg = dict(CFG, loss=loss, **kw)
    cfg["transformer_config"] = dict(CFG["transformer_config"], mask_type=mask_type)
    return cfg


def picked(g, stride):
    return g if g.numel() <= 20000 else g.flatten()[::stride]


def block_mask(center, start, num_mask):
    """_mask_center_block (P/:268-294) for given start indices."""
    rows = []
    for pts, i in zip(center, start):
        d = torch.norm(pts[int(i)].reshape(1, 1, 3) - pts.unsqueeze(0), p=2, dim=-1)
        idx = torch.argsort(d, dim=-1, descending=False)[0]
        m = torch.zeros(len(idx))
        m[idx[:num_mask]] = 1
        rows.append(m.bool())
    return torch.stack(rows)


class PointMAERef(FrozenPointMAE):
    """The oracle's frozen Point-MAE (same state-dict keys) with the pre-training forward added."""

    def __init__(self, loss="cdl2"):
        super().__init__()
        self.group_divider = R.Group(64, 32)
        self.loss_func = O.ChamferDistanceL2(reduction="mean") if loss == "cdl2" else O.ChamferDistanceL1()

    def forward(self, pts, mask):
        neighborhood, center, _ = self.group_divider(pts)
        enc = self.MAE_encoder
        tokens = enc.encoder(neighborhood)
        B, _, C = tokens.shape
        x_vis = tokens[~mask].reshape(B, -1, C)
        pos = enc.pos_embed(center[~mask].reshape(B, -1, 3))
        x_vis = enc.norm(enc.blocks(x_vis, pos))
        pos_vis = self.decoder_pos_embed(center[~mask]).reshape(B, -1, C)
        pos_mask = self.decoder_pos_embed(center[mask]).reshape(B, -1, C)
        N = pos_mask.shape[1]
        x_full = torch.cat([x_vis, self.mask_token.expand(B, N, -1)], dim=1)
        x_rec = self.MAE_decoder(x_full, torch.cat([pos_vis, pos_mask], dim=1), N)[:, -N:]
        rebuild = self.increase_dim(x_rec.transpose(1, 2)).transpose(1, 2).reshape(B * N, -1, 3)
        return self.loss_func(rebuild, neighborhood[mask].reshape(B * N, -1, 3))

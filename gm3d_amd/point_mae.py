"""Point_MAE -- the plain Point-MAE pre-training model of the reference (Point-MAE_SA3D/models/Point_MAE.py:216-441), used by
the published GM3D run as the FROZEN feature/point teacher (P/main_pretrain.py:302-328, config_m.yaml: mask_ratio 0).
Same constructor (`config` with group_size, num_group, loss, transformer_config.{mask_ratio, mask_type, trans_dim,
encoder_dims, depth, drop_path_rate, num_heads, decoder_depth, decoder_num_heads}) and state-dict keys
(MAE_encoder.{encoder,pos_embed,blocks,norm}.*, mask_token, decoder_pos_embed.*, MAE_decoder.*, increase_dim.*).
"""
import numpy as np
import torch
import torch.nn as nn

from . import models_mae_learn_loss as M
from .models_mae_learn_loss import Encoder, Group, TransformerDecoder, TransformerEncoder, split_ids, take
from .models_mae_learn_loss_Classifier_SVM_feature_besed import _pos_mlp
from .ops import ChamferDistanceL1, ChamferDistanceL2


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


class MaskTransformer(nn.Module):
    """P/models/Point_MAE.py:216-337.  forward -> (x_vis, bool mask)."""

    def __init__(self, config, **kwargs):
        super().__init__()
        tc = _get(config, "transformer_config")
        self.mask_ratio, self.mask_type = _get(tc, "mask_ratio"), _get(tc, "mask_type")
        self.trans_dim, self.depth = _get(tc, "trans_dim"), _get(tc, "depth")
        self.drop_path_rate, self.num_heads = _get(tc, "drop_path_rate"), _get(tc, "num_heads")
        self.encoder_dims = _get(tc, "encoder_dims")
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        self.pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, self.trans_dim))
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(embed_dim=self.trans_dim, depth=self.depth, drop_path_rate=dpr,
                                         num_heads=self.num_heads)
        self.norm = nn.LayerNorm(self.trans_dim)

    def _mask_center_rand(self, center, noaug=False, rng=np.random):
        """P/:296-317: exactly int(mask_ratio*G) masked groups per cloud, uniformly at random (host shuffle like the reference)."""
        B, G, _ = center.shape
        if noaug or self.mask_ratio == 0:
            return torch.zeros(B, G, dtype=torch.bool, device=center.device)
        num_mask = int(self.mask_ratio * G)
        out = np.zeros([B, G])
        for i in range(B):
            m = np.hstack([np.zeros(G - num_mask), np.ones(num_mask)])
            rng.shuffle(m)
            out[i] = m
        return torch.from_numpy(out).to(torch.bool).to(center.device)

    def _mask_center_block(self, center, noaug=False, rng=np.random):
        """P/:268-294: the int(mask_ratio*G) groups nearest to a random centre."""
        B, G, _ = center.shape
        if noaug or self.mask_ratio == 0:
            return torch.zeros(B, G, dtype=torch.bool, device=center.device)
        start = torch.as_tensor(rng.randint(0, G, size=B), device=center.device)
        d = torch.norm(center[torch.arange(B, device=center.device), start].unsqueeze(1) - center, p=2, dim=-1)
        idx = torch.argsort(d, dim=-1)[:, :int(self.mask_ratio * G)]
        mask = torch.zeros(B, G, dtype=torch.bool, device=center.device)
        mask.scatter_(1, idx, True)
        return mask

    device_mask = False      # True: the mask and the id lists come from gm3d_mask_centers (no host shuffle, no host-to-device copy)

    def select(self, center, noaug=False, mask_noise=None, mask_start=None, mask=None):
        """-> (mask (B,G) bool, vis_ids, mask_ids, on_device).  An explicit `mask` overrides everything.  With device_mask (or
        injected draws) on a GPU the two id lists are the halves of gm3d_mask_centers' [visible | masked] order and nothing here
        talks to the host: mask_noise (B,G) f32 ranks the groups of `rand`, mask_start (B) int32 names the start centres of
        `block`; draws that are not given come from torch.rand / torch.randint on the device (graph-safe Philox, like
        generate_mask's noise).  Otherwise: the reference's host-side draw."""
        B, G, _ = center.shape
        off = noaug or self.mask_ratio == 0
        num_mask = 0 if off else int(self.mask_ratio * G)
        if mask is not None:
            mask = mask.to(center.device, torch.bool)
            return (mask,) + split_ids(mask, G - num_mask) + (False,)
        if center.is_cuda and not off and (self.device_mask or mask_noise is not None or mask_start is not None):
            from . import heads
            if self.mask_type == "rand":
                noise = torch.rand(B, G, device=center.device) if mask_noise is None else mask_noise
                mask, order = heads.mask_centers(noise, num_mask)
            else:
                start = (torch.randint(0, G, (B,), device=center.device, dtype=torch.int32) if mask_start is None else mask_start)
                mask, order = heads.mask_centers(center, num_mask, start=start)
            return mask, order[:, :G - num_mask], order[:, G - num_mask:], True
        mask = (self._mask_center_rand if self.mask_type == "rand" else self._mask_center_block)(center, noaug=noaug)
        return (mask,) + split_ids(mask, G - num_mask) + (False,)

    def forward(self, neighborhood, center, noaug=False, mask_noise=None, mask_start=None, mask=None):
        mask, vis_ids, _, _ = self.select(center, noaug, mask_noise, mask_start, mask)
        tokens = self.encoder(neighborhood)
        pos = _pos_mlp(self.pos_embed, center)
        return self.blocks(take(tokens, vis_ids), take(pos, vis_ids), norm=self.norm), mask


class Point_MAE(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        tc = _get(config, "transformer_config")
        self.trans_dim = _get(tc, "trans_dim")
        self.MAE_encoder = MaskTransformer(config)
        self.group_size, self.num_group = _get(config, "group_size"), _get(config, "num_group")
        self.drop_path_rate = _get(tc, "drop_path_rate")
        self.mask_token = nn.Parameter(torch.zeros(1, 1, self.trans_dim))
        self.decoder_pos_embed = nn.Sequential(nn.Linear(3, 128), nn.GELU(), nn.Linear(128, self.trans_dim))
        self.decoder_depth, self.decoder_num_heads = _get(tc, "decoder_depth"), _get(tc, "decoder_num_heads")
        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.decoder_depth)]
        self.MAE_decoder = TransformerDecoder(embed_dim=self.trans_dim, depth=self.decoder_depth, drop_path_rate=dpr,
                                              num_heads=self.decoder_num_heads)
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        self.increase_dim = nn.Sequential(nn.Conv1d(self.trans_dim, 3 * self.group_size, 1))
        nn.init.trunc_normal_(self.mask_token, std=0.02)
        self.loss = _get(config, "loss")
        self.build_loss_func(self.loss)

    def build_loss_func(self, loss_type):
        if loss_type == "cdl1":
            self.loss_func = ChamferDistanceL1()
        elif loss_type == "cdl2":
            self.loss_func = ChamferDistanceL2(reduction="mean")
        else:
            raise NotImplementedError

    def _points(self, x_rec):
        c = self.increase_dim[0]
        if M.FUSED_HEADS and x_rec.is_cuda:
            from . import heads
            return heads.LinearBiasFn.apply(x_rec, c.weight, c.bias, heads._adt())
        return nn.functional.linear(x_rec, c.weight.squeeze(-1), c.bias)

    def _rebuild(self, neighborhood, center, mask_noise=None, mask_start=None, mask=None, chosen=None):
        """select -> encoder on the visible tokens -> decoder -> point head.
        -> (mask, vis_ids, mask_ids, pred (B,M,3k), chosen).  chosen: the replayable path (see forward); None: decided by the arguments."""
        enc = self.MAE_encoder
        if chosen is None:
            chosen = mask is not None or mask_noise is not None or mask_start is not None or enc.device_mask
        mask, vis_ids, mask_ids, _ = enc.select(center, False, mask_noise, mask_start, mask)
        B, N = mask_ids.shape
        tokens = enc.encoder(neighborhood)
        pos = _pos_mlp(enc.pos_embed, center)
        dpos = _pos_mlp(self.decoder_pos_embed, center)
        if chosen and M.FUSED_HEADS and center.is_cuda:
            from . import heads
            tok_vis, pos_vis, _ = heads.token_assemble(tokens, pos, vis_ids, mask_ids)
            _, pos_full = heads.pos_assemble(dpos, vis_ids, mask_ids, dt=tok_vis.dtype)
            x_vis = enc.blocks(tok_vis, pos_vis, norm=enc.norm)
            x_full = torch.cat([x_vis, heads.ExpandRowsFn.apply(self.mask_token, B, N, x_vis.dtype)], dim=1)
        else:
            x_vis = enc.blocks(take(tokens, vis_ids), take(pos, vis_ids), norm=enc.norm)
            x_full = torch.cat([x_vis, self.mask_token.expand(B, N, -1).to(x_vis.dtype)], dim=1)
            pos_full = torch.cat([take(dpos, vis_ids), take(dpos, mask_ids)], dim=1)
        x_rec = self.MAE_decoder(x_full, pos_full, N)[:, -N:]          # P/:212: only the masked tokens are decoded to points
        pred = self._points(x_rec)
        if chosen and M.FUSED_HEADS:
            pred = pred.contiguous()
        return mask, vis_ids, mask_ids, pred, chosen

    def _patch_loss(self, pred, neighborhood, mask_ids, chosen):
        """-> (the loss of P/:425-426, its per-patch values (B,M) when the fused patch kernel formed them, else None)."""
        B, N = mask_ids.shape
        if chosen and M.FUSED_HEADS:
            from . import heads
            if heads.patch_chamfer_loss_supported(pred, neighborhood, mask_ids):
                # cdl2: mean(d1) + mean(d2) over equal-sized patches = the mean of the per-point d1 + d2 the GM3D loss kernel forms
                fn = heads.PatchChamferLossFn if self.loss == "cdl2" else heads.PatchChamferL1LossFn
                return fn.apply(pred, neighborhood, mask_ids)
        rebuild = pred.reshape(B * N, -1, 3).float()
        gt = take(neighborhood, mask_ids).reshape(B * N, -1, 3)
        return self.loss_func(rebuild, gt), None

    def forward(self, pts, noaug=False, vis=False, mask_noise=None, mask_start=None, mask=None, **kwargs):
        """P/:391-441 (Point-MAE pre-training loss).  mask / mask_noise / mask_start: see MaskTransformer.select.  With any of them
        (or MAE_encoder.device_mask) on a GPU the step is the replayable one: token and position gathers through
        heads.token_assemble / pos_assemble, the loss through the fused patch kernels.
        vis=True (P/:428-439): no loss; -> (ret1 (1,B*G*k,3): all clouds' visible patches then all rebuilt ones, back at their centres,
        ret2 (1,B*V*k,3): the visible part, a view of ret1's head, full_center (B*G,3): all masked centres then all visible ones),
        assembled by ops.reconstruct_assemble(flat=True) for any B and returned detached: the launch has no backward."""
        neighborhood, center, _ = self.group_divider(pts)
        if noaug:
            return self.MAE_encoder(neighborhood, center, noaug=True)[0]
        mask, vis_ids, mask_ids, pred, chosen = self._rebuild(neighborhood, center, mask_noise, mask_start, mask)
        if vis:
            from . import ops
            p = pred if pred.stride(1) == pred.shape[2] and pred.stride(2) == 1 else pred.contiguous()
            dense, full_center = ops.reconstruct_assemble(p, neighborhood, center, vis_ids, mask_ids, flat=True)
            ret1 = dense.unsqueeze(0)
            return ret1, ret1[:, :pts.shape[0] * vis_ids.shape[1] * self.group_size], full_center
        return self._patch_loss(pred, neighborhood, mask_ids, chosen)[0]

    @torch.no_grad()
    def features_decoder(self, neighborhood, center, features, mask_ids):
        """forward_features_dino_decoder (P/engine_pretrain_Classifier_SVM.py:669-687) for the all-visible teacher:
        -> (features of all G tokens (B,G,C), their decoded points (B,G,3k), points decoded from the student's `features`
        (B,M,C) placed at the masked centres (B,M,3k))."""
        x_vis, _ = self.MAE_encoder(neighborhood, center, noaug=True)
        dpos = _pos_mlp(self.decoder_pos_embed, center)
        G = x_vis.shape[1]
        pts_org = self._points(self.MAE_decoder(x_vis, dpos, G))
        pts_rec = self._points(self.MAE_decoder(features, take(dpos, mask_ids), G))
        return x_vis, pts_org, pts_rec

"""Point-M2AE classifiers: the hierarchical encoder of point_m2ae.PointM2AE, one final LayerNorm and the fine-tune head, for the
ModelNet40 and ScanObjectNN rows of the published Point-M2AE + GeoMask3D results (Point-M2AE_SA3D/cfgs/finetune_modelnet_PointM2AE.yaml,
config_finetune_scan_*_PointM2AE.yaml; logs in Point-M2AE_SA3D/log_files/).

The reference ships no Point-M2AE source.  Its fine-tune logs carry the keys of the Point-MAE driver (main_finetune.py:471-474), so
the runs used that driver and engine_finetune.py, which engine_finetune mirrors here.  The published parameter counts fix the
architecture: log_files/modelnet40.txt reports 12,830,056 and log_files/hardest.txt 12,921,935 = the encoder here (token_embed +
encoder_pos_embeds + encoder_blocks: 12,653,632) + LayerNorm(384) (768) + the head Linear(F,256) BN ReLU Dropout(0.5)
Linear(256,256) BN ReLU Dropout(0.5) Linear(256,cls) with F = 384 (ModelNet40, 40 classes: 175,656) or F = 768 (ScanObjectNN,
15 classes: 267,535).  Choices the sources do not fix, stated once:

  * x = the final norm applied to the coarsest level's encoder output (B, 64, 384) with nothing masked at ANY level: each level's
    attention mask is its radius mask alone and every token is encoded (PointM2AE(pts, noaug=True) back-projects an all-visible
    coarse mask, which still hides the finer tokens no coarser group contains; the two agree bit for bit when every one is covered);
  * ModelNet40 feature = x.mean(1) + x.max(1)[0] (Point-M2AE's SVM feature, validate.pool_features); ScanObjectNN feature =
    cat([x.mean(1), x.max(1)[0]], -1);
  * the max-pool's gradient goes to the lowest token index among tied maxima.

What of the yaml's `model` section is read: NAME, group_sizes, num_groups, encoder_depths, encoder_dims, local_radius, drop_path_rate,
num_heads, cls_dim and `smooth` (finetune_modelnet_PointM2AE.yaml:73 sets 0.3; the ScanObjectNN yamls set none).  A non-zero `smooth`
makes the model's own loss (loss_ce, get_loss_acc) losses.SmoothLoss(smooth) -- Point-M2AE's smoothed cross-entropy, on-value
1 - smooth, off-value smooth / (cls_dim - 1) --; absent or 0 it is nn.CrossEntropyLoss().  The fine-tune engine takes its criterion
from the caller: engine_finetune.build_criterion(model) hands out the loss this config asks for.  Nothing else of the yaml (optimizer,
scheduler, dataset, batch size, clipping) is read here; the engine's arguments carry those.

GPU: the tail (pooling, head, both training-mode BatchNorms with their running statistics, Dropout) is ops.cls_tail -- two launches
forward, two backward (gm3d_amd/csrc/cls_tail.hip); the Dropout factors come from one graph-safe device draw.  FUSED_TAIL = False
runs the same tail as PyTorch modules (the CPU path and the cross-check).
"""
import torch
import torch.nn as nn

from . import ops
from .hierarchical_group import HierarchicalGroup
from .point_m2ae import BlockStack, LayerNorm, TokenEmbed, _pos_mlp, encode_levels
from .point_transformer import PointTransformer, _cfg, strip_pretrain_prefixes

FUSED_TAIL = True          # the tail on gm3d_cls_tail_fwd / _bwd (tests and tools/bench_m2ae_finetune.py flip it)

POOL_MODES = {"meansum": 0, "cat": 1}
_ENCODER_DEFAULTS = dict(group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5], encoder_dims=[96, 192, 384],
                         local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6)
_keep_cache = {}


def dropout_factors(B, probs, device):
    """The factors of the head's two Dropout layers for a batch of B: (2,B,256) f32, 0 or 1 / (1 - p), from ONE uniform draw and one
    launch (gm3d_drop_path_scales: floor(keep + u) / keep, the DropPath draw).  None when both probabilities are 0."""
    if all(p == 0.0 for p in probs):
        return None
    if any(not 0.0 <= p < 1.0 for p in probs):
        raise NotImplementedError("Dropout probabilities in [0, 1)")
    key = (tuple(probs), str(device))
    keep = _keep_cache.get(key)
    if keep is None:       # built once, outside any stream capture (the eager warm-up steps come first)
        keep = torch.tensor([1.0 - p for p in probs], dtype=torch.float32).to(device)
        _keep_cache[key] = keep
    u = torch.rand(2, B * 256, dtype=torch.float32, device=device)
    out = torch.empty_like(u)
    from ._capi import lib
    ops._launch("gm3d_drop_path_scales", {"S": 2, "B": B * 256}, lib.gm3d_drop_path_scales, ops._ptr(u), ops._ptr(keep), 2, B * 256,
                ops._ptr(out), ops._stream())
    return out.view(2, B, 256)


class PointM2AEClassifier(nn.Module):
    """config: the `model` section of a Point-M2AE fine-tune yaml plus `cls_dim` (dict or attribute object).
    pool: "meansum" (ModelNet40) or "cat" (ScanObjectNN).  State-dict keys: the pretraining keys of every encoder parameter,
    norm.* (the final LayerNorm) and cls_head_finetune.{0,1,4,5,8}.*."""

    def __init__(self, config, pool="meansum"):
        super().__init__()
        if pool not in POOL_MODES:
            raise ValueError("pool must be one of %s" % sorted(POOL_MODES))
        c = dict(_ENCODER_DEFAULTS)
        c.update({k: _cfg(config, k) for k in c if (k in config if isinstance(config, dict) else hasattr(config, k))})
        self.config, self.cfg, self.pool = config, c, pool
        self.cls_dim = _cfg(config, "cls_dim")
        dims, depths = c["encoder_dims"], c["encoder_depths"]
        assert len(dims) == 3, "built for the three-scale configuration"
        self.num_heads = c["num_heads"]
        self.local_radius = list(c["local_radius"])
        self.group_divider = HierarchicalGroup(c["num_groups"], c["group_sizes"])
        self.token_embed = nn.ModuleList([TokenEmbed(3 if i == 0 else dims[i - 1], dims[i]) for i in range(3)])
        self.encoder_pos_embeds = nn.ModuleList([_pos_mlp(d) for d in dims])
        dpr = [x.item() for x in torch.linspace(0, c["drop_path_rate"], sum(depths))]
        self.encoder_blocks, at = nn.ModuleList(), 0
        for d, n in zip(dims, depths):
            self.encoder_blocks.append(BlockStack(d, n, self.num_heads, dpr[at:at + n]))
            at += n
        self.norm = LayerNorm(dims[2])
        feat = dims[2] * (2 if pool == "cat" else 1)
        self.cls_head_finetune = nn.Sequential(
            nn.Linear(feat, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim))
        has = "smooth" in config if isinstance(config, dict) else hasattr(config, "smooth")
        self.smooth = float(_cfg(config, "smooth") or 0.0) if has else 0.0
        self.build_loss_func()

    def build_loss_func(self):
        """nn.CrossEntropyLoss(), or losses.SmoothLoss(smooth) when the config sets a non-zero `smooth`."""
        if self.smooth:
            from .losses import SmoothLoss
            self.loss_ce = SmoothLoss(self.smooth)
        else:
            self.loss_ce = nn.CrossEntropyLoss()

    def get_loss_acc(self, ret, gt):
        loss = self.loss_ce(ret, gt.long())
        pred = ret.argmax(-1)
        acc = (pred == gt).sum() / float(gt.size(0))
        return loss, acc * 100

    # ------------------------------------------------------------------ checkpoints
    def load_pretrained_state(self, state_dict):
        """state_dict: a PointM2AE pre-training checkpoint's 'state_dict' / 'model' / 'ema_state_dict' / 'base_model' entry; the
        coarsest level's encoder norm (encoder_norms.2.*) becomes norm.*.  -> the `_IncompatibleKeys` of load_state_dict(strict=False):
        missing = cls_head_finetune.*, unexpected = the decoder, the loss predictor, mask_token and encoder_norms.{0,1}."""
        sd = {}
        for k, v in strip_pretrain_prefixes(state_dict).items():
            sd["norm." + k[len("encoder_norms.2."):] if k.startswith("encoder_norms.2.") else k] = v
        return self.load_state_dict(sd, strict=False)

    def load_model_from_ckpt(self, bert_ckpt_path, key="base_model"):
        """PointTransformer.load_model_from_ckpt's pattern: None -> fresh initialisation; else the file's first present entry of
        key / 'base_model' / 'state_dict' / 'model', read with torch.load(weights_only=True)."""
        if bert_ckpt_path is None:
            self.apply(PointTransformer._init_weights)
            return None
        ckpt = torch.load(bert_ckpt_path, map_location="cpu", weights_only=True)
        if key not in ckpt:
            key = next(k for k in ("base_model", "state_dict", "model") if k in ckpt)
        return self.load_pretrained_state(ckpt[key])

    # ------------------------------------------------------------------ forward
    def forward_tokens(self, pts, group=None):
        """-> (B, 64, 384): the final norm of the coarsest level's encoder output, nothing masked.  group: the grouping
        (neighbourhoods, centres, idxs) when the caller has it already."""
        neighborhoods, centers, idxs = group if group is not None else self.group_divider(pts)
        enc = encode_levels(self, neighborhoods, centers, idxs, None)
        return self.norm(enc[2])

    def forward_features(self, x):
        """tokens (B,T,C) -> the pooled feature, as PyTorch ops (the FUSED_TAIL = False path)."""
        mean, mx = x.mean(1), x.max(1)[0]
        return mean + mx if self.pool == "meansum" else torch.cat([mean, mx], dim=-1)

    def forward(self, pts):
        x = self.forward_tokens(pts)
        if FUSED_TAIL and x.is_cuda:
            head = self.cls_head_finetune
            drop = dropout_factors(x.shape[0], (head[3].p, head[7].p), x.device) if self.training else None
            return ops.cls_tail(x.contiguous(), head, POOL_MODES[self.pool], self.training, drop=drop)
        return self.cls_head_finetune(self.forward_features(x))


class Point_M2AE_ModelNet40(PointM2AEClassifier):
    def __init__(self, config, **kwargs):
        super().__init__(config, pool="meansum")


class Point_M2AE_ScanObjectNN(PointM2AEClassifier):
    def __init__(self, config, **kwargs):
        super().__init__(config, pool="cat")


MODELS = {"Point_M2AE_ModelNet40": Point_M2AE_ModelNet40, "Point_M2AE_ScanObjectNN": Point_M2AE_ScanObjectNN}


def build_model(config):
    """The classifier a fine-tune yaml's `model` section names (config.NAME)."""
    name = _cfg(config, "NAME")
    if name not in MODELS:
        raise KeyError("unknown Point-M2AE classifier %r (known: %s)" % (name, sorted(MODELS)))
    return MODELS[name](config)

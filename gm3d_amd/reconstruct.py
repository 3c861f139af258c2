"""The reconstruction pass: what a pre-trained masked autoencoder rebuilds, as dense clouds.

The reference reaches this only through Point_MAE.forward(..., vis=True) (Point-MAE_SA3D/models/Point_MAE.py:428-439) and its tester
(tools/runner.py::test), one cloud at a time.  Here the whole batch is assembled by one launch (ops.reconstruct_assemble) in the
per-cloud layout -- cloud b of `dense` is [its visible patches | its rebuilt patches], centres in the same order -- together with the
mask that was drawn, the per-patch loss of the fused patch-loss kernel and the Chamfer distance of every dense cloud to its input.

reconstruct          plain Point-MAE (gm3d_amd.point_mae.Point_MAE)
reconstruct_geomask  GeoMask3D (models_mae_learn_loss.MaskedAutoencoderViT): teacher pass -> guided mask -> student -> loss, the
                     forward half of engine_pretrain.step_forward_backward without augmentation and without backward; adds the
                     student's and the teacher's predicted per-patch loss, to be ranked against the real one.
reconstruct_m2ae     Point-M2AE + GeoMask3D (gm3d_amd.point_m2ae.PointM2AE): the forward half of point_m2ae.pretrain_forward without
                     augmentation and without backward.  The visible count of the finer levels differs from cloud to cloud, so the
                     clouds are ragged: ops.reconstruct_partition (one launch per level) puts every cloud's visible patches first and
                     states the count per cloud.
All run in eval mode under no_grad; bf16=True is the autocast of validate.extract_features.  Everything returned is detached.
Point-M2AE's reconstruction is the dense level-1 cloud (what its decoder rebuilds) and the level-0 split of the input points.
"""
import torch

from . import ops
from .models_mae_learn_loss import split_ids, take


class Reconstruction:
    """dense (B,G*k,3): per cloud [visible patches | rebuilt patches], each patch back at its centre; n_visible = V*k, so the visible
    cloud is dense[:, :n_visible]; center (B,G,3) in the same order (centre i belongs to rows i*k .. i*k+k-1); mask (B,G) bool
    (True = masked), vis_ids (B,V), mask_ids (B,M); pred (B,M,3k): the decoder's centre-relative patches; patch_loss (B,M): the
    model's own loss per masked patch, loss: its mean (what forward returns); cd_l2 / cd_l1 (B): ChamferDistanceL2 / L1 between each
    dense cloud and its input.  GeoMask3D adds loss_pred (B,M) and teacher_loss_pred (B,G)."""

    def __init__(self, **kw):
        self.loss_pred = self.teacher_loss_pred = None
        self.__dict__.update(kw)

    @property
    def visible(self):
        return self.dense[:, :self.n_visible]

    def __repr__(self):
        return "Reconstruction(B=%d, points=%d, n_visible=%d)" % (self.dense.shape[0], self.dense.shape[1], self.n_visible)


def _raw(model):
    return model.module if hasattr(model, "module") else model


def cloud_chamfer(dense, pts):
    """-> (cd_l2 (B), cd_l1 (B)): the reference's ChamferDistanceL2 / L1 (extensions/chamfer_dist) per cloud pair, through the general
    Chamfer kernel (P = B, n = dense points, m = input points)."""
    d1, d2, _, _ = ops.chamfer(dense.contiguous(), pts.contiguous())
    return d1.mean(1) + d2.mean(1), (d1.sqrt().mean(1) + d2.sqrt().mean(1)) / 2


def _patch_matrix(pred, neighborhood, mask_ids, l1):
    """per-patch loss through the general Chamfer kernel, for patch sizes the fused patch kernel does not take"""
    B, M = mask_ids.shape
    d1, d2, _, _ = ops.chamfer(pred.reshape(B * M, -1, 3).float().contiguous(), take(neighborhood, mask_ids).reshape(B * M, -1, 3))
    m = (d1.sqrt().mean(1) + d2.sqrt().mean(1)) / 2 if l1 else d1.mean(1) + d2.mean(1)
    return m.reshape(B, M)


def _assemble(pts, pred, neighborhood, center, mask, vis_ids, mask_ids, matrix, loss, **extra):
    B, G, k, _ = neighborhood.shape
    dense, full_center = ops.reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=False)
    dense = dense.view(B, G * k, 3)
    cd_l2, cd_l1 = cloud_chamfer(dense, pts)
    return Reconstruction(dense=dense, n_visible=vis_ids.shape[1] * k, center=full_center.view(B, G, 3), mask=mask, vis_ids=vis_ids,
                          mask_ids=mask_ids, pred=pred.detach(), patch_loss=matrix.detach(), loss=loss.detach(), cd_l2=cd_l2,
                          cd_l1=cd_l1, **extra)


@torch.no_grad()
def reconstruct(model, pts, mask=None, mask_noise=None, mask_start=None, bf16=False):
    """Plain Point-MAE: pts (B,N,3) on the GPU -> Reconstruction.  The mask comes from MaskTransformer.select: `mask` (B,G) bool,
    `mask_noise` (B,G) f32 for `rand`, `mask_start` (B) int32 for `block`, MAE_encoder.device_mask, or the reference's host draw.
    With any of the device forms nothing here talks to the host (the pass can be captured in a graph)."""
    raw = _raw(model)
    was_training = raw.training
    raw.eval()
    try:
        pts = pts.float().contiguous()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            neighborhood, center, _ = raw.group_divider(pts)
            mask, vis_ids, mask_ids, pred, _ = raw._rebuild(neighborhood, center, mask_noise, mask_start, mask, chosen=True)
            if mask_ids.shape[1] == 0:
                raise ValueError("nothing is masked (mask_ratio 0): there is nothing to reconstruct")
            loss, matrix = raw._patch_loss(pred, neighborhood, mask_ids, True)
            if matrix is None:
                matrix = _patch_matrix(pred, neighborhood, mask_ids, raw.loss == "cdl1")
        return _assemble(pts, pred, neighborhood, center, mask, vis_ids, mask_ids, matrix, loss)
    finally:
        raw.train(was_training)


@torch.no_grad()
def reconstruct_geomask(model, teacher, pts, epoch, total_epoch, mask_ratio, mask_noise=None, bf16=False):
    """GeoMask3D: the student `model` and its EMA `teacher` (the module, or an engine_pretrain.ModelEma) on pts (B,N,3)
    -> Reconstruction with loss_pred (B,M), the student's predicted loss of the masked patches in mask_ids order, and
    teacher_loss_pred (B,G), what the mask was guided by.  mask_noise (B,G) f32: the draw that ranks the unguided groups (fresh
    uniforms on the device when None).  The sequence is engine_pretrain.step_forward_backward's: group once, all-visible teacher pass,
    generate_mask_ids, student, forward_loss."""
    from .engine_pretrain import _all_false, _arange_ids
    raw, teacher = _raw(model), getattr(teacher, "ema", teacher)
    was_training = raw.training, teacher.training
    raw.eval()
    teacher.eval()
    try:
        pts = pts.float().contiguous()
        B, L, dev = pts.shape[0], raw.num_group, pts.device
        len_keep = int(L * (1 - mask_ratio))
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            group = teacher.group_divider(pts)
            all_ids = (_arange_ids(B, L, dev), _arange_ids(B, 0, dev))
            outs_ema = teacher(pts, mask=_all_false(B, L, dev), num_visible=L, group=group, need_pix_pred=False, ids=all_ids)
            if pts.is_cuda and L <= 512:
                _, vis_ids, mask_ids, mask = teacher.generate_mask_ids(outs_ema["loss_pred"], mask_ratio=mask_ratio, guide=True,
                                                                       epoch=epoch, total_epoch=total_epoch, noise=mask_noise,
                                                                       want_bool=True)
            else:
                mask = teacher.generate_mask(outs_ema["loss_pred"], mask_ratio=mask_ratio, guide=True, epoch=epoch,
                                             total_epoch=total_epoch, noise=mask_noise).flatten(1).to(torch.bool)
                vis_ids, mask_ids = split_ids(mask, len_keep)
            outs = raw(pts, mask=mask, num_visible=len_keep, group=group, ids=(vis_ids, mask_ids))
            M = outs["mask_num"]
            if M == 0:
                raise ValueError("nothing is masked (mask_ratio %r): there is nothing to reconstruct" % (mask_ratio,))
            pred = outs["pix_pred"][:, -M:]
            loss_outs = raw.forward_loss(pred, outs["neighborhood"], mask, mask_ids=mask_ids, full_pred=outs["pix_pred"])
        return _assemble(pts, pred, outs["neighborhood"], outs["center"], mask, vis_ids, mask_ids, loss_outs["matrix"],
                         loss_outs["Chamfer_mean"], loss_pred=outs["loss_pred"][:, -M:].float(),
                         teacher_loss_pred=outs_ema["loss_pred"].float())
    finally:
        raw.train(was_training[0])
        teacher.train(was_training[1])


class M2AEReconstruction:
    """What the hierarchical model rebuilds.  Level 1 (G1 tokens of k1 points, the decoder's target): dense (B,G1*k1,3), per cloud
    [visible patches | rebuilt patches], each part in ascending token index and every patch back at its centre; n_visible (B,) int32
    counts the visible level-1 TOKENS of each cloud -- the visible part of cloud b is dense[b, :n_visible[b]*k1] --; center (B,G1,3)
    and order (B,G1) int32 (the token at each slot) in the same order.  Level 0 (the raw input points the encoder saw, then the hidden
    ones): points0 (B,G0*k0,3) with n_visible0 (B,) in level-0 tokens.  mask (B,G_last) bool over the coarsest tokens and masks, its
    back-projection per level; rec (B,G1,k1,3): the decoder's centre-relative patches for every level-1 token; per_token (B,G1): the
    Chamfer loss of every level-1 patch; patch_loss (B,G_last): forward_loss's `matrix`; loss: its mean over the masked level-1 tokens;
    loss_pred (B,G_last): the student's predicted loss, teacher_loss_pred the teacher's (None without a teacher); vis_overflow: the
    (1,) int32 device flag of the visible-first order; cd_l2 / cd_l1 (B): ChamferDistanceL2 / L1 between each dense cloud and its
    input, cd_l2_target / cd_l1_target (B): the same against the level-0 centres -- level-1 patches are made of level-0 centres, so
    that is the set the decoder aims at.
    visible(b) / visible0(b) read one count back to the host: they are for looking at a result, outside the pass."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def visible(self, b):
        return self.dense[b, :int(self.n_visible[b]) * (self.dense.shape[1] // self.order.shape[1])]

    def visible0(self, b):
        return self.points0[b, :int(self.n_visible0[b]) * (self.points0.shape[1] // self.masks[0].shape[1])]

    def __repr__(self):
        return "M2AEReconstruction(B=%d, points=%d, points0=%d)" % (self.dense.shape[0], self.dense.shape[1], self.points0.shape[1])


@torch.no_grad()
def reconstruct_m2ae(model, pts, teacher=None, epoch=0, total_epoch=1, mask=None, mask_noise=None, bf16=False):
    """Point-M2AE + GeoMask3D: the student `model` and its EMA `teacher` (the module, or an engine_pretrain.ModelEma) on pts (B,N,3)
    -> M2AEReconstruction.  The sequence is point_m2ae.pretrain_forward's: group_stage without augmentation, all-visible teacher pass,
    generate_mask_ids with the model's own mask_ratio (mask_noise (B,G_last) f32 ranks the unguided tokens; fresh uniforms on the
    device when None), student with vis_count, forward_loss.  With a teacher nothing here talks to the host (the pass can be captured
    in a graph).  teacher=None: `mask` (B,G_last) bool is taken as it is; it is a caller's input and is checked on the host once
    (something must be masked), and the visible-first order then keeps every row (no static bound is known)."""
    from . import masked_stack
    from . import models_mae_learn_loss as M
    from . import point_m2ae as P
    raw, teacher = _raw(model), getattr(teacher, "ema", teacher)
    if teacher is None and mask is None:
        raise ValueError("without a teacher an explicit mask (B,%d) bool is required" % raw.num_group)
    was_training = raw.training, teacher is not None and teacher.training
    raw.eval()
    if teacher is not None:
        teacher.eval()
    try:
        pts = pts.float().contiguous()
        B = pts.shape[0]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            _, group, prop = P.group_stage((teacher if teacher is not None else raw).group_divider, pts, augment=False)
            if teacher is not None:
                t = teacher(pts, mask=None, group=group, prop=prop)
                m, vis_ids, mask_ids = M.generate_mask_ids(t["loss_pred"], mask_ratio=raw.mask_ratio, guide=True, epoch=epoch,
                                                           total_epoch=total_epoch, noise=mask_noise)
                if mask_ids.shape[1] == 0:
                    raise ValueError("nothing is masked (mask_ratio %r): there is nothing to reconstruct" % (raw.mask_ratio,))
                mask, vis_count = m.to(torch.bool), vis_ids.shape[1]
            else:
                mask, vis_count = mask.to(pts.device, torch.bool).contiguous(), None
                if tuple(mask.shape) != (B, raw.num_group):
                    raise ValueError("mask must be (B,%d) bool, got %s" % (raw.num_group, tuple(mask.shape)))
                if not bool(mask.any()):
                    raise ValueError("nothing is masked: there is nothing to reconstruct")
            out = raw(pts, mask=mask, group=group, vis_count=vis_count, prop=prop)
            lo = raw.forward_loss(out["rec"], group[0], group[2], out["masks"])
        neighborhoods, centers, _ = group
        masks, rec = out["masks"], out["rec"]
        G1, k1 = rec.shape[1], rec.shape[2]
        dense, center, order, n_visible = ops.reconstruct_partition(rec.reshape(B, G1, 3 * k1), neighborhoods[1], centers[1], masks[1])
        points0, _, _, n_visible0 = ops.reconstruct_partition(None, neighborhoods[0], centers[0], masks[0])
        cd_l2, cd_l1 = cloud_chamfer(dense, pts)
        cd_l2_target, cd_l1_target = cloud_chamfer(dense, centers[0])
        return M2AEReconstruction(dense=dense, n_visible=n_visible, center=center, order=order, points0=points0, n_visible0=n_visible0,
                                  mask=mask, masks=masks, rec=rec.detach(), per_token=lo["per_token"].detach(),
                                  patch_loss=lo["matrix"].detach(), loss=lo["Chamfer_mean"].detach(),
                                  loss_pred=out["loss_pred"].detach().float(),
                                  teacher_loss_pred=None if teacher is None else t["loss_pred"].detach().float(),
                                  vis_overflow=masked_stack.overflow_flag(pts.device), cd_l2=cd_l2, cd_l1=cd_l1,
                                  cd_l2_target=cd_l2_target, cd_l1_target=cd_l1_target)
    finally:
        raw.train(was_training[0])
        if teacher is not None:
            teacher.train(was_training[1])

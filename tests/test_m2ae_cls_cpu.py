"""CPU: the Point-M2AE classifiers (gm3d_amd/point_m2ae_cls.py) -- architecture pinned by the published parameter counts, checkpoint
key mapping, model registry, optimizer groups, and the host-side shape guards of the classification-tail entry points."""
import ctypes

import pytest
import torch

# the `model` sections of Point-M2AE_SA3D/cfgs/finetune_modelnet_PointM2AE.yaml and config_finetune_scan_hardest_PointM2AE.yaml
MODELNET = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], smooth=0.3,
                encoder_depths=[5, 5, 5], encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1,
                num_heads=6, cls_dim=40)
SCAN = dict(NAME="Point_M2AE_ScanObjectNN", group_sizes=[32, 16, 16], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
            encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=15)


def _n_params(m):
    return sum(p.numel() for p in m.parameters())


def test_parameter_counts_match_the_published_logs():
    """n_parameters of Point-M2AE_SA3D/log_files/modelnet40.txt (12,830,056) and log_files/hardest.txt (12,921,935)."""
    from gm3d_amd import point_m2ae_cls as C
    assert _n_params(C.PointM2AEClassifier(MODELNET, pool="meansum")) == 12830056
    assert _n_params(C.PointM2AEClassifier(SCAN, pool="cat")) == 12921935


def test_build_model_dispatches_on_name():
    from gm3d_amd import point_m2ae_cls as C
    m = C.build_model(MODELNET)
    assert isinstance(m, C.Point_M2AE_ModelNet40) and m.pool == "meansum" and m.cls_dim == 40
    s = C.build_model(SCAN)
    assert isinstance(s, C.Point_M2AE_ScanObjectNN) and s.pool == "cat" and s.cls_dim == 15
    assert s.group_divider.group_sizes == (32, 16, 16)
    assert s.cls_head_finetune[0].in_features == 768 and m.cls_head_finetune[0].in_features == 384
    with pytest.raises(KeyError):
        C.build_model(dict(MODELNET, NAME="Point_M2AE_ShapeNetPart"))


def test_pretrained_state_loads_with_the_stated_key_sets():
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_m2ae import PointM2AE
    torch.manual_seed(0)
    pre = PointM2AE()
    sd = {"module." + k: v for k, v in pre.state_dict().items()}          # a DDP checkpoint's prefix is stripped
    m = C.build_model(MODELNET)
    res = m.load_pretrained_state(sd)
    assert res.missing_keys and all(k.startswith("cls_head_finetune.") for k in res.missing_keys)
    # (BatchNorm fills in a missing num_batches_tracked itself when the dict carries no version metadata)
    assert set(res.missing_keys) == {k for k in m.state_dict() if k.startswith("cls_head_finetune.")
                                     and not k.endswith("num_batches_tracked")}
    dead = ("h_decoder.", "decoder_pos_embeds.", "token_prop.", "decoder_norm.", "rec_head.", "loss_pred_head.", "encoder_norms.0.",
            "encoder_norms.1.")
    want_unexpected = {k for k in pre.state_dict() if k.startswith(dead) or k == "mask_token"}
    assert set(res.unexpected_keys) == want_unexpected
    psd, msd = pre.state_dict(), m.state_dict()
    for k, v in msd.items():
        if k.startswith("cls_head_finetune."):
            continue
        src = "encoder_norms.2." + k[len("norm."):] if k.startswith("norm.") else k
        assert torch.equal(v, psd[src]), k


def test_load_model_from_ckpt_reads_a_saved_pretraining_checkpoint(tmp_path):
    from gm3d_amd import checkpoint
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_m2ae import PointM2AE
    torch.manual_seed(1)
    pre = PointM2AE()
    path = str(tmp_path / "m2ae.pth")
    checkpoint.save_checkpoint(path, pre, epoch=3, model_name="Point_M2AE")
    m = C.build_model(SCAN)
    res = m.load_model_from_ckpt(path)
    assert all(k.startswith("cls_head_finetune.") for k in res.missing_keys)
    assert torch.equal(m.norm.weight, pre.encoder_norms[2].weight)
    assert torch.equal(m.encoder_blocks[2].blocks[4].mlp.fc2.weight, pre.encoder_blocks[2].blocks[4].mlp.fc2.weight)


def test_optimizer_groups_lr_scale_one_and_no_decay_on_1d():
    """param_groups_lrd: no classifier parameter name starts with `blocks`, so every group has lr scale 1; weight decay 0 exactly for
    the 1-D parameters."""
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import point_m2ae_cls as C
    m = C.build_model(MODELNET)
    groups = EF.param_groups_lrd(m, weight_decay=0.05, layer_decay=0.75)
    assert all(g["lr_scale"] == 1.0 for g in groups)
    seen = 0
    for g in groups:
        for n, p in zip(g["names"], g["params"]):
            assert g["weight_decay"] == (0.0 if p.ndim == 1 else 0.05), n
            seen += 1
    assert seen == len(list(m.parameters()))
    opt = EF.build_optimizer(m, lr=5e-4, weight_decay=0.05)
    assert all(g["lr_scale"] == 1.0 for g in opt.param_groups)
    assert sum(len(g["params"]) for g in opt.param_groups) == seen
    for g in opt.param_groups:
        assert g["weight_decay"] == (0.0 if all(p.ndim == 1 for p in g["params"]) else 0.05)


def test_cpu_forward_uses_the_module_tail():
    """On the CPU the classifier's tail is the PyTorch head: the pooled feature has the stated form."""
    from gm3d_amd import point_m2ae_cls as C
    m = C.build_model(SCAN)
    x = torch.randn(3, 64, 384)
    f = m.forward_features(x)
    assert torch.equal(f, torch.cat([x.mean(1), x.max(1)[0]], -1))
    m2 = C.build_model(MODELNET)
    assert torch.equal(m2.forward_features(x), x.mean(1) + x.max(1)[0])


# ------------------------------------------------------------------ C-ABI guards of gm3d_cls_tail_fwd / _bwd (never dereferenced)
ONE = ctypes.c_void_p(16)


def _fwd(B=40, T=64, C=384, mode=0, cls_dim=40, training=1, dtype=0):
    from gm3d_amd._capi import lib
    return lib.gm3d_cls_tail_fwd(ONE, B, T, C, mode, *([ONE] * 10), cls_dim, *([ONE] * 6), 1e-5, 0.1, training, None, None,
                                 *([ONE] * 5), None, dtype, None)


def _bwd(B=40, T=64, C=384, mode=0, cls_dim=40, training=1, dtype=0):
    from gm3d_amd._capi import lib
    return lib.gm3d_cls_tail_bwd(B, T, C, mode, *([ONE] * 7), cls_dim, training, None, None, *([ONE] * 5), ONE, None, ONE, ONE,
                                 *([ONE] * 10), dtype, None)


REFUSED = [
    ("B=129", dict(B=129)),
    ("C=256", dict(C=256)),
    ("C=768", dict(C=768)),
    ("T=513", dict(T=513)),
    ("cls_dim=257", dict(cls_dim=257)),
    ("mode=2", dict(mode=2)),
    ("mode=-1", dict(mode=-1)),
    ("dtype=2", dict(dtype=2)),
]


@pytest.mark.parametrize("fn", [_fwd, _bwd], ids=["fwd", "bwd"])
@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shapes_return_unsupported_before_any_launch(fn, row):
    from gm3d_amd._capi import GM3D_EUNSUPPORTED
    assert fn(**row[1]) == GM3D_EUNSUPPORTED


@pytest.mark.parametrize("fn", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_last_accepted_shapes_pass_the_guard_with_an_empty_batch(fn):
    """B = 0 returns right after the shape checks: the largest accepted T, cls_dim and both modes are OK without a launch."""
    from gm3d_amd._capi import GM3D_OK
    for kw in (dict(T=512), dict(cls_dim=256), dict(mode=1), dict(dtype=1)):
        assert fn(B=0, **kw) == GM3D_OK, kw
    assert fn(B=0, T=0) != GM3D_OK and fn(B=0, cls_dim=0) != GM3D_OK


def test_training_needs_two_rows_and_aligned_weights():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, lib
    assert _fwd(B=1, training=1) == GM3D_EINVAL and _bwd(B=1, training=1) == GM3D_EINVAL
    odd = ctypes.c_void_p(20)
    assert lib.gm3d_cls_tail_fwd(ONE, 4, 64, 384, 0, *([ONE] * 4), odd, *([ONE] * 5), 40, *([ONE] * 6), 1e-5, 0.1, 1, None, None,
                                 *([ONE] * 5), None, 0, None) == GM3D_EUNSUPPORTED


def test_header_states_the_limits():
    import os
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gm3d.h")).read()
    assert "C == 384, 1 <= T <= 512, B <= 128 (B >= 2 in training), 1 <= cls_dim <= 256, mode 0 or 1" in txt

"""CPU: soft targets for the classification fine-tune (gm3d_amd/losses.py, its wiring in engine_finetune / point_m2ae_cls) -- the C-ABI
symbols, both smoothing conventions against fp64 closed forms, compact against dense targets, the CPU mixup against the reference's
expression, the model's `smooth` key, build_criterion's switch and the mixup type check."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the `model` section of Point-M2AE_SA3D/cfgs/finetune_modelnet_PointM2AE.yaml, without its `smooth` (the tests add it)
MODELNET = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
                encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=40)

LOGITS = torch.tensor([[1.5, -0.25, 0.75, 3.0, -2.0],
                       [0.1, 0.2, -0.3, 0.4, 2.5],
                       [-1.0, 4.0, 0.5, -0.5, 1.25]])
LABELS = torch.tensor([3, 0, 2])


def _closed_form(on, off, logits=LOGITS, labels=LABELS):
    """fp64: mean_i sum_c t_ic (-log p_ic) with t = off everywhere and on at the label"""
    logp = F.log_softmax(logits.double(), dim=-1)
    t = torch.full_like(logp, off)
    t[torch.arange(len(labels)), labels] = on
    return float((-(t * logp).sum(-1)).mean())


def test_the_three_symbols_are_declared_with_the_headers_argument_counts():
    from gm3d_amd import _capi, build
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gm3d.h")).read(), flags=re.S)
    for name in ("gm3d_soft_ce_fwd", "gm3d_soft_ce_bwd", "gm3d_mixup_points"):
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert name in _capi.SIGNATURES and len(_capi.SIGNATURES[name]) == len(params.split(",")), name
    assert [len(_capi.SIGNATURES[n]) for n in ("gm3d_soft_ce_fwd", "gm3d_soft_ce_bwd", "gm3d_mixup_points")] == [12, 12, 9]
    assert build.SOURCES["soft_ce.hip"] == ["-ffp-contract=off"]


def test_both_smoothing_conventions_equal_their_closed_forms_and_differ():
    from gm3d_amd import losses as L
    C = LOGITS.size(1)
    timm = float(L.LabelSmoothingCrossEntropy(0.1)(LOGITS, LABELS))
    m2ae = float(L.SmoothLoss(0.3)(LOGITS, LABELS))
    assert timm == pytest.approx(_closed_form(1 - 0.1 + 0.1 / C, 0.1 / C), rel=1e-6)
    assert m2ae == pytest.approx(_closed_form(1 - 0.3, 0.3 / (C - 1)), rel=1e-6)
    # timm's own statement of it: (1 - s) * nll + s * mean_c(-log p)
    logp = F.log_softmax(LOGITS.double(), -1)
    nll = -logp[torch.arange(3), LABELS]
    assert timm == pytest.approx(float((0.9 * nll + 0.1 * (-logp.mean(-1))).mean()), rel=1e-6)
    # the two conventions are different losses, also at the same strength
    assert abs(float(L.SmoothLoss(0.1)(LOGITS, LABELS)) - timm) > 1e-3 * timm
    assert abs(m2ae - timm) > 1e-3 * timm
    ce = float(F.cross_entropy(LOGITS, LABELS))
    assert float(L.LabelSmoothingCrossEntropy(0.0)(LOGITS, LABELS)) == pytest.approx(ce, rel=1e-6)
    assert float(L.SmoothLoss(0.0)(LOGITS, LABELS)) == pytest.approx(ce, rel=1e-6)
    with pytest.raises(ValueError):
        L.SmoothLoss(0.3)(LOGITS[:, :1], torch.zeros(3, dtype=torch.long))


def test_soft_target_cross_entropy_has_timms_semantics_and_gradient():
    from gm3d_amd import losses as L
    g = torch.Generator().manual_seed(1)
    t = torch.rand(3, 5, generator=g) * 0.7                    # rows that do not sum to 1
    z = LOGITS.clone().requires_grad_(True)
    loss = L.SoftTargetCrossEntropy()(z, t)
    want = torch.sum(-t.double() * F.log_softmax(LOGITS.double(), -1), -1).mean()
    assert float(loss.detach()) == pytest.approx(float(want), rel=1e-6)
    loss.backward()
    zd = LOGITS.double().requires_grad_(True)
    torch.sum(-t.double() * F.log_softmax(zd, -1), -1).mean().backward()
    assert float((z.grad.double() - zd.grad).abs().max()) <= 1e-6 * float(zd.grad.abs().max())


@pytest.mark.parametrize("lam", [0.3, 0.0, 1.0])
def test_compact_form_equals_dense_form(lam):
    from gm3d_amd import losses as L
    ya = torch.tensor([3, 0, 2])
    yb = torch.tensor([1, 0, 4])                               # row 1: ya == yb
    crit = L.LabelSmoothingCrossEntropy(0.1)
    wa, wb, u = (float(v) for v in crit.coefficients(5, lam))
    dense = torch.full((3, 5), u)
    dense[torch.arange(3), ya] += wa
    dense[torch.arange(3), yb] += wb
    assert dense.sum(-1).numpy() == pytest.approx(np.ones(3), rel=1e-6)
    za, zb = LOGITS.clone().requires_grad_(True), LOGITS.clone().requires_grad_(True)
    a = L.soft_cross_entropy(za, ya=ya, yb=yb, coef=torch.tensor([wa, wb, u]))
    b = L.soft_cross_entropy(zb, dense=dense)
    assert float(a.detach()) == pytest.approx(float(b.detach()), rel=1e-6)
    a.backward()
    b.backward()
    assert float((za.grad - zb.grad).abs().max()) <= 1e-6 * float(zb.grad.abs().max())
    # the loss object on MixedTargets is the same thing
    mixed = L.MixedTargets(ya, yb, torch.tensor([lam, 1 - lam], dtype=torch.float32), lam)
    assert float(crit(LOGITS, mixed)) == pytest.approx(float(b.detach()), rel=1e-6)
    with pytest.raises(ValueError):
        L.soft_cross_entropy(LOGITS, ya=ya, coef=torch.zeros(3), dense=dense)
    with pytest.raises(ValueError):
        L.soft_cross_entropy(LOGITS)


def test_an_out_of_range_label_makes_its_row_nan_on_the_cpu_path_too():
    from gm3d_amd import losses as L
    assert torch.isnan(L.LabelSmoothingCrossEntropy(0.1)(LOGITS, torch.tensor([3, 5, 2])))


def test_cpu_mixup_equals_the_reference_expression():
    from gm3d_amd import losses as L
    g = torch.Generator().manual_seed(2)
    data = torch.randn(4, 33, 3, generator=g)
    labels = torch.tensor([7, 1, 1, 12])
    perm = torch.tensor([2, 0, 3, 1])
    mix = L.PointMixup(0.2)
    for lam in (0.37, 1.0, 0.0):
        mix.draw(4, lam=lam, perm=perm)
        out, tgt = mix.mix(data, labels)
        assert torch.equal(out, lam * data + (1 - lam) * data[perm])
        assert torch.equal(tgt.ya, labels) and torch.equal(tgt.yb, labels[perm]) and tgt.lam == lam
        dense = tgt.dense(15)
        assert dense.shape == (4, 15) and dense.sum(-1).numpy() == pytest.approx(np.ones(4), rel=1e-6)
        if lam == 1.0:
            assert torch.equal(out.view(torch.int32), data.view(torch.int32))
    # the draws: lam from rng.beta(alpha, alpha), then torch.randperm(B) -- the reference's order and calls
    rng, gen = np.random.RandomState(5), torch.Generator().manual_seed(6)
    lam, p = L.PointMixup(0.2, rng=rng, generator=gen).draw(4)
    assert lam == np.random.RandomState(5).beta(0.2, 0.2)
    assert torch.equal(p, torch.randperm(4, generator=torch.Generator().manual_seed(6)))
    with pytest.raises(ValueError):
        mix.draw(4, lam=0.5, perm=torch.tensor([0, 1, 2, 4]))


def test_the_m2ae_classifier_reads_smooth_from_its_config():
    from gm3d_amd import losses as L
    from gm3d_amd import point_m2ae_cls as C
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(6, 40, generator=g)
    gt = torch.tensor([0, 39, 7, 7, 12, 3])
    m = C.Point_M2AE_ModelNet40(dict(MODELNET, smooth=0.3))
    assert isinstance(m.loss_ce, L.SmoothLoss) and m.loss_ce.eps == 0.3
    loss, acc = m.get_loss_acc(logits, gt)
    assert torch.equal(loss, L.SmoothLoss(0.3)(logits, gt))
    assert float(acc) == float((logits.argmax(-1) == gt).sum() / 6.0 * 100)
    for cfg in (MODELNET, dict(MODELNET, smooth=0), SimpleNamespace(**MODELNET)):
        plain = C.Point_M2AE_ModelNet40(cfg)
        assert type(plain.loss_ce) is nn.CrossEntropyLoss
        assert torch.equal(plain.get_loss_acc(logits, gt)[0], nn.CrossEntropyLoss()(logits, gt))
    plain.smooth = 0.2
    plain.build_loss_func()
    assert isinstance(plain.loss_ce, L.SmoothLoss) and plain.loss_ce.eps == 0.2
    assert not any("loss_ce" in k for k in m.state_dict())


def test_build_criterion_has_three_branches():
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import losses as L
    model = SimpleNamespace(config=dict(MODELNET, smooth=0.3))
    c = EF.build_criterion(model, SimpleNamespace(smoothing=0.1))          # the model's config wins
    assert isinstance(c, L.SmoothLoss) and c.eps == 0.3
    c = EF.build_criterion(SimpleNamespace(config=MODELNET), SimpleNamespace(smoothing=0.1))
    assert isinstance(c, L.LabelSmoothingCrossEntropy) and c.smoothing == 0.1
    for model, args in ((None, None), (SimpleNamespace(config=MODELNET), SimpleNamespace(smoothing=0.0)), (nn.Linear(2, 2), SimpleNamespace())):
        assert type(EF.build_criterion(model, args)) is nn.CrossEntropyLoss


def test_a_mixup_that_is_no_point_mixup_is_refused():
    from gm3d_amd import engine_finetune as EF
    with pytest.raises(TypeError):
        EF.train_one_epoch(nn.Linear(2, 2), nn.CrossEntropyLoss(), [], None, "cpu", 0, mixup_fn=object())
    with pytest.raises(TypeError):
        EF.finetune_step(None, None, None, None, None, mixup=lambda x, y: (x, y))

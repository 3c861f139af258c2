"""-m gpu: one EAGER step of every model with every `empty` allocation poisoned (tests/poison.py) -- B = 4, DropPath 0, mask noise
injected, no graph.  Loss, the flat gradient buffer (every parameter gradient), the updated parameters, the Adam moments, the EMA
teacher and the BatchNorm buffers must equal the unpoisoned step bit for bit under NaN, +inf and -inf; the voting evaluations their
votes, means and predictions.  A difference means a kernel of that step read memory nobody wrote.  The last test is the coverage
condition over the allocation sites of gm3d_amd/."""
from contextlib import nullcontext
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import model_ref as R
from tests import clouds, poison
from tests import point_mae_ref as PR
from tests.poison import assert_same, poisoned

pytestmark = pytest.mark.gpu
PATTERNS = ["nan", "+inf", "-inf"]
B = 4
M2AE_MODELNET = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
                     encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=40)
FT_CFG = dict(trans_dim=384, depth=12, drop_path_rate=0.0, cls_dim=40, num_heads=6, group_size=32, num_group=64, encoder_dims=384)
RAN = set()          # the cases of this module that ran to their end (the coverage test runs only after all of them)


def _no_drop(m):
    for mod in m.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    return m


def _state(model, opt, out, keys):
    """what a step leaves behind, cloned: the named outputs, the flat gradients / parameters / moments (/ teacher), BatchNorm buffers"""
    res = {k: out[k].detach().clone() for k in keys}
    res["grad"], res["param"], res["exp_avg"], res["exp_avg_sq"] = opt.G.clone(), opt.P.clone(), opt.M.clone(), opt.V.clone()
    res["shadow"] = opt.PS.clone()
    if opt.E is not None:
        res["ema"], res["ema_shadow"] = opt.E.clone(), opt.ES.clone()
    res["bn"] = {k: v.detach().clone() for k, v in model.named_buffers() if "running_" in k or "num_batches_tracked" in k}
    assert res["bn"]
    return res


# ------------------------------------------------------------------------------------------------------------------ the steps
def geomask3d(bf16, f32_own=False):
    def run(ctx):
        from gm3d_amd import engine_pretrain as E
        from gm3d_amd import gemm
        from gm3d_amd import models_mae_learn_loss as M
        torch.manual_seed(0)
        m = _no_drop(R.det_fill_(M.mae_vit_base_patch16_dec512d8b(), seed=0)).cuda().train()
        ema = E.ModelEma(m, 0.999)
        opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema)
        args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=bf16, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
        noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(1)).cuda()
        x = clouds.uniform(B, 1024, 50).cuda()
        was = gemm.F32_OWN
        gemm.F32_OWN = f32_own
        try:
            with ctx:
                o = E.pretrain_step(m, ema, opt, x, 200, args, mask_noise=noise, augment=False)
                torch.cuda.synchronize()
        finally:
            gemm.F32_OWN = was
        return _state(m, opt, o, ("loss_chfr", "loss_learn", "grad_norm", "mask", "matrix", "teacher_loss_pred"))
    return run


def point_mae(mask_type, bf16):
    def run(ctx):
        from gm3d_amd import engine_pretrain_point_mae as EP
        from gm3d_amd.point_mae import Point_MAE
        torch.manual_seed(0)
        m = _no_drop(R.det_fill_(Point_MAE(PR.config(mask_type, "cdl2")), seed=41)).cuda().train()
        opt = EP.build_optimizer(m)
        args = SimpleNamespace(bf16=bf16, lr=1e-3, epochs=300, warmup_epochs=10, step_per_update=1)
        noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(2)).cuda()
        start = torch.tensor([3, 63, 0, 17], dtype=torch.int32).cuda()
        x = clouds.gaussian(B, 1024, seed=500).cuda()
        with ctx:
            o = EP.pretrain_step(m, opt, x, args, mask_noise=noise, mask_start=start, augment=False, micro_step=0)
            torch.cuda.synchronize()
        return _state(m, opt, o, ("loss", "grad_norm"))
    return run


def point_m2ae(bf16):
    def run(ctx):
        from gm3d_amd import engine_pretrain as E
        from gm3d_amd import point_m2ae as P
        torch.manual_seed(11)
        m = _no_drop(P.PointM2AE()).cuda().train()
        ema = E.ModelEma(m, 0.999)
        opt = E.build_optimizer(m, lr=1e-3, flat=True, model_ema=ema)
        args = SimpleNamespace(bf16=bf16, epochs=300)
        noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(40)).cuda()
        x = clouds.gaussian(B, 2048, seed=900).cuda()
        with ctx:
            o = P.pretrain_step(m, ema, opt, x, 100, args, mask_noise=noise, augment=False)
            torch.cuda.synchronize()
        assert int(o["vis_overflow"]) == 0
        return _state(m, opt, o, ("loss", "loss_chfr", "loss_learn", "grad_norm"))
    return run


def _point_transformer():
    from gm3d_amd.point_transformer import PointTransformer
    torch.manual_seed(0)
    return _no_drop(R.det_fill_(PointTransformer(dict(FT_CFG)), seed=5)).cuda()


def _m2ae_classifier():
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_m2ae import PointM2AE
    cfg = M2AE_MODELNET
    pre = PointM2AE({k: v for k, v in cfg.items() if k in ("group_sizes", "num_groups", "encoder_depths", "encoder_dims", "local_radius",
                                                            "num_heads")})
    R.det_fill_(pre, seed=3)
    torch.manual_seed(3)
    m = C.build_model(cfg)
    m.load_pretrained_state(pre.state_dict())
    return _no_drop(m).cuda()


def finetune(make, bf16):
    def run(ctx):
        from gm3d_amd import engine_finetune as EF
        m = make().train()
        opt = EF.build_optimizer(m, lr=5e-4, flat=True, max_norm=10.0)
        pts = clouds.gaussian(B, 2048, seed=21).cuda()
        targets = torch.tensor([1, 5, 39, 0]).cuda()
        subset = np.random.RandomState(3).choice(1200, 1024, False)
        with ctx:
            o = EF.finetune_step(m, nn.CrossEntropyLoss(), opt, pts, targets, npoints=1024, max_norm=10.0, bf16=bf16, subset=subset,
                                 augment=False)
            torch.cuda.synchronize()
        return _state(m, opt, o, ("loss", "grad_norm", "outputs"))
    return run


def vote(make, bf16):
    def run(ctx):
        from gm3d_amd import engine_finetune as EF
        m = make().eval()
        pts = clouds.gaussian(B, 2048, seed=33)
        labels = torch.tensor([1, 5, 39, 0])
        with ctx:
            o = EF.validate_vote(m, [(None, None, (pts, labels))], "cuda", npoints=1024, times=3, bf16=bf16,
                                 rng=np.random.RandomState(7), graphed=False, outputs=True)
            torch.cuda.synchronize()
        return {"pred": o["pred"], "mean": o["mean"], "votes": o["votes"], "acc_vote": o["acc_vote"], "n": o["n"]}
    return run


STEPS = {
    "geomask3d-bf16": geomask3d(True),
    "geomask3d-fp32": geomask3d(False),
    "geomask3d-fp32-own": geomask3d(False, f32_own=True),
    "point_mae-rand": point_mae("rand", True),
    "point_mae-block": point_mae("block", True),
    "point_mae-rand-fp32": point_mae("rand", False),
    "point_m2ae-bf16": point_m2ae(True),
    "finetune-point_mae-bf16": finetune(_point_transformer, True),
    "finetune-point_mae-fp32": finetune(_point_transformer, False),
    "finetune-point_m2ae-bf16": finetune(_m2ae_classifier, True),
    "finetune-point_m2ae-fp32": finetune(_m2ae_classifier, False),
    "vote-point_mae": vote(_point_transformer, True),
    "vote-point_m2ae": vote(_m2ae_classifier, True),
}
_plain = {}


def plain(name):
    """the unpoisoned step, computed once per model and left unchanged; run twice, since a bitwise comparison under poison presupposes
    that the step repeats itself bitwise (every reduction of these steps has a fixed order)"""
    if name not in _plain:
        a, b = STEPS[name](nullcontext()), STEPS[name](nullcontext())
        assert_same(a, b, name + " plain-vs-plain")
        _plain[name] = a
    return _plain[name]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("name", list(STEPS))
def test_step_does_not_depend_on_unwritten_memory(name, pattern):
    want = plain(name)
    ctx = poisoned(pattern)
    got = STEPS[name](ctx)
    ps = ctx.state
    assert poison._active[0] is None
    print("%s / %s: %d poisoned allocations, %d from %d sites of gm3d_amd/" % (name, pattern, ps.count, ps.recorded, len(ps.sites)))
    assert ps.recorded >= 1, "no allocation of gm3d_amd/ was poisoned: a vacuous case"
    assert_same(want, got, "%s[%s]" % (name, pattern))
    RAN.add((name, pattern))


EXPECTED = {(n, p) for n in STEPS for p in PATTERNS}
poison.CASES[__name__] = (RAN, EXPECTED)


def test_every_allocation_site_is_reached_or_listed():
    """The coverage condition (tests/poison.py coverage): judged once this module ran whole; `every line reached or listed` over the
    union of both poison modules when both ran whole in this process (as the suite runs them), the list's own rules in any case."""
    if RAN != EXPECTED:
        pytest.skip("judged after the whole module ran (%d of %d cases did)" % (len(RAN), len(EXPECTED)))
    complete = all(ran == exp for ran, exp in poison.CASES.values()) and len(poison.CASES) == 2
    print("allocation sites: %d scanned, %d reached, %d listed (complete: %s)" % (poison.coverage(complete) + (complete,)))

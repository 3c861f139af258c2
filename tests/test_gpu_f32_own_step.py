"""-m gpu: the fp32 (parity) mode with gemm.F32_OWN = True -- every dense product of the step on csrc/gemm_f32.hip.

 * no library product: torch.mm / addmm / matmul / bmm / baddbmm / F.linear / Tensor.__matmul__ replaced by functions that raise, one
   fp32 forward + backward + optimizer step of GeoMask3D pretraining, plain Point-MAE pretraining and the fine-tune step completes;
   with the switch off the same patched step raises (the patch looks at the right thing);
 * the reference fixtures' 1e-5 bars hold on the new kernels (the existing fixture tests' own code, run with the switch on);
 * replay == eager and run-to-run, as equalities."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import model_ref as R
from tests import clouds

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


class LibraryProduct(RuntimeError):
    pass


@pytest.fixture
def own(monkeypatch):
    from gm3d_amd import gemm
    monkeypatch.setattr(gemm, "F32_OWN", True)
    return gemm


def forbid_library_products(monkeypatch):
    def raiser(name):
        def f(*a, **k):
            raise LibraryProduct(name)
        return f
    for name in ("mm", "addmm", "matmul", "bmm", "baddbmm"):
        monkeypatch.setattr(torch, name, raiser("torch." + name))
    monkeypatch.setattr(torch.nn.functional, "linear", raiser("F.linear"))
    monkeypatch.setattr(torch.Tensor, "__matmul__", raiser("Tensor.__matmul__"))


def _geomask(B, seed=0):
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    torch.manual_seed(0)
    m = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(), seed=seed).cuda().train()
    for mod in m.modules():
        if isinstance(mod, M.DropPath):
            mod.drop_prob = 0.0
    ema = E.ModelEma(m, 0.999)
    opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema)
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=False, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
    return E, m, ema, opt, args


def _geomask_step(B=2):
    E, m, ema, opt, args = _geomask(B)
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(1)).cuda()
    before = opt.P.clone()
    o = E.pretrain_step(m, ema, opt, clouds.uniform(B, 1024, 50).cuda(), 200, args, mask_noise=noise, augment=False)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o[k])) for k in ("loss_chfr", "loss_learn", "grad_norm"))
    assert not torch.equal(opt.P, before)


def _point_mae(B=4, G=64):
    from gm3d_amd import engine_pretrain_point_mae as EP
    from tests.test_gpu_point_mae_pretrain import _model
    m = _model("rand", drop_path=0.0, num_group=G)
    opt = EP.build_optimizer(m)
    args = SimpleNamespace(bf16=False, lr=1e-3, epochs=300, warmup_epochs=10, step_per_update=1)
    return EP, m, opt, args


def _point_mae_step(B=4):
    EP, m, opt, args = _point_mae(B)
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(2)).cuda()
    before = opt.P.clone()
    o = EP.pretrain_step(m, opt, clouds.gaussian(B, 1024, seed=500).cuda(), args, mask_noise=noise, augment=False, micro_step=0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o["loss"])) and not torch.equal(opt.P, before)


def _finetune_step(B=4):
    from gm3d_amd import engine_finetune as EF
    from tests.test_gpu_finetune import build
    pm = build(seed=5, drop_path=0.0).train()
    opt = EF.build_optimizer(pm, lr=5e-4)
    pts = clouds.gaussian(B, 2048, seed=21).cuda()
    targets = torch.tensor([1, 5, 39, 0][:B]).cuda()
    subset = np.random.RandomState(3).choice(1200, 1024, False)
    before = {k: v.detach().clone() for k, v in pm.named_parameters()}
    res = EF.finetune_step(pm, nn.CrossEntropyLoss(), opt, pts, targets, npoints=1024, max_norm=10.0, bf16=False, subset=subset,
                           augment=False)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(res["loss"]))
    assert any(not torch.equal(v, before[k]) for k, v in pm.named_parameters())


STEPS = {"geomask3d": _geomask_step, "point_mae": _point_mae_step, "finetune": _finetune_step}


@pytest.mark.parametrize("which", list(STEPS))
def test_fp32_step_issues_no_library_product(which, own, monkeypatch):
    forbid_library_products(monkeypatch)
    STEPS[which]()


@pytest.mark.parametrize("which", list(STEPS))
def test_the_patch_catches_the_library_path_with_the_switch_off(which, monkeypatch):
    from gm3d_amd import gemm
    assert gemm.F32_OWN is False
    forbid_library_products(monkeypatch)
    with pytest.raises(LibraryProduct):
        STEPS[which]()


# --------------------------------------------------------------------------- reference parity on the new kernels
def test_geomask3d_fixture_parity_b2_uniform(own, monkeypatch):
    from gm3d_amd import models_mae_learn_loss as M
    from tests.test_gpu_model import _fixture_case
    torch.manual_seed(0)
    model = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(norm_pix_loss=False), seed=0).cuda()
    _fixture_case(M, model, np.load(os.path.join(GOLD, "pretrain_b2_uniform.npz")), monkeypatch, "b2_uniform")


def test_point_mae_fixture_parity_b4(own, monkeypatch):
    from gm3d_amd import models_mae_learn_loss as M
    from tests import point_mae_ref as PR
    from tests.test_gpu_point_mae_pretrain import test_fp32_parity_with_the_reference_fixture as check
    fx = np.load(os.path.join(GOLD, "point_mae_pretrain_b4.npz"))
    for case in PR.CASES:
        check(M, fx, case, monkeypatch)


def test_finetune_fixture_parity_b4(own, monkeypatch):
    from gm3d_amd import models_mae_learn_loss as M
    from tests.test_gpu_finetune import test_against_reference_fixture as check
    check(M, True, monkeypatch)


# --------------------------------------------------------------------------- replay == eager, run to run
def _geomask_trajectory(graphed, B=2):
    E, m, ema, opt, args = _geomask(B)
    pool = [clouds.uniform(B, 1024, 60 + i).cuda() for i in range(3)]
    noise = [torch.rand(B, 64, generator=torch.Generator().manual_seed(10 + i)).cuda() for i in range(6)]
    for i in range(3):          # the eager warm-up of a captured step: optimizer steps on both sides
        E.pretrain_step(m, ema, opt, pool[i].clone(), 200, args, mask_noise=noise[i], augment=False)
    g = E.GraphedPretrainStep(m, ema, opt, args, pool[0], 200, warmup_iters=0, augment=False, inject_mask_noise=True) if graphed else None
    outs = []
    for i in range(3, 6):
        if graphed:
            o = g(pool[i % 3], noise[i])
        else:
            o = E.pretrain_step(m, ema, opt, pool[i % 3].clone(), 200, args, mask_noise=noise[i], augment=False)
        outs += [o["loss_chfr"].clone(), o["loss_learn"].clone(), o["grad_norm"].clone()]
    torch.cuda.synchronize()
    return outs + [opt.P.clone()]


def test_geomask3d_fp32_replay_equals_eager_and_eager_repeats(own):
    a, b, c = _geomask_trajectory(False), _geomask_trajectory(False), _geomask_trajectory(True)
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "two eager runs from the same state differ"
    assert all(torch.equal(x, y) for x, y in zip(a, c)), [float(x.float().sub(y.float()).abs().max()) for x, y in zip(a, c)]


def test_point_mae_fp32_replay_equals_eager_and_eager_repeats(own):
    B, G = 4, 64
    EP, m, opt, args = _point_mae(B, G)
    x = [clouds.gaussian(B, 1024, seed=500 + i).cuda() for i in range(3)]
    gen = torch.Generator().manual_seed(17)
    noise = [torch.rand(B, G, generator=gen).cuda() for _ in range(3)]
    g = EP.GraphedPointMAEStep(m, opt, x[0], args, warmup_iters=2, augment=False, inject_mask_noise=True)
    state = ({k: v.clone() for k, v in m.state_dict().items()}, opt.M.clone(), opt.V.clone(), opt.step_dev.clone())

    def restore():
        with torch.no_grad():
            m.load_state_dict(state[0])
            opt.M.copy_(state[1]); opt.V.copy_(state[2]); opt.step_dev.copy_(state[3])
            opt.sync_shadows()
            if opt.GA is not None:
                opt.GA.zero_()

    def eager():
        restore()
        out = []
        for i in range(3):
            o = EP.pretrain_step(m, opt, x[i].clone(), args, mask_noise=noise[i], augment=False, micro_step=i)
            out += [o["loss"].clone(), o["grad_norm"].clone(), opt.P.clone()]
        return out

    a, b = eager(), eager()
    restore()
    c = []
    for i in range(3):
        o = g(x[i], mask_noise=noise[i])
        c += [o["loss"].clone(), o["grad_norm"].clone(), opt.P.clone()]
    assert all(bool(torch.isfinite(t).all()) for t in a)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two eager runs from the same state differ"
    assert all(torch.equal(p, q) for p, q in zip(a, c)), [float(p.float().sub(q.float()).abs().max()) for p, q in zip(a, c)]
    assert not torch.equal(a[2], a[8])

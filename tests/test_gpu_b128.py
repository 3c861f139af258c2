"""-m gpu: BASELINE config #2 AT ITS REAL SIZE -- B=128 clouds, N=1024, G=64, k=32, bf16, hipGraph replay: the configuration the
headline clouds/s figure of bench.py comes from (the other step tests run B=2..16).

  * FPS centres and KNN neighbourhoods of all 128 clouds bit-exact against the CPU oracle;
  * every generated mask row has exactly 39 masked / 25 visible tokens;
  * 6 replayed steps == 6 eager steps on the same inputs (the size-dependent failure mode found in round 1 -- torch's multi-block
    reduce_kernel returning stale values under replay above ~64k elements, engine_pretrain.GraphedPretrainStep -- only shows at
    full size);
  * the bf16 step's losses sit within the bf16 band of an fp32 eager step on identical inputs / noise;
  * all 251 gradients of the bf16 step, its teacher loss_pred and loss matrix against the fp32 step's, each within 3 x the reference's
    own bf16-autocast error at this size, plus the tile check of tests/parity.py; the guided mask at epoch 200 on clouds without a near-tie.
Randomness is removed as in tests/test_gpu_graph.py (DropPath off, augmentation off, mask noise injected)."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import clouds

pytestmark = pytest.mark.gpu

B = 128


def _args(bf16):
    return SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=bf16, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)


def _build(flat=True):
    from gm3d_amd import engine_pretrain as E, models_mae_learn_loss as M
    torch.manual_seed(0)
    m = M.mae_vit_base_patch16_dec512d8b().cuda().train()
    for mod in m.modules():
        if isinstance(mod, M.DropPath):
            mod.drop_prob = 0.0
    ema = E.ModelEma(m, 0.999)
    opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema) if flat else E.build_optimizer(m, lr=2e-4)
    return m, ema, opt


def test_grouping_of_128_clouds_bit_exact(oracle_ops):
    from gm3d_amd import models_mae_learn_loss as M
    x = clouds.uniform(B, 1024, 7)
    nb, cen, nbo = M.Group(64, 32)(x.cuda())
    fidx = oracle_ops.furthest_point_sample(x, 64)
    rcen = torch.gather(x, 1, fidx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    _, ri = oracle_ops.knn(x, rcen, 32)
    rnb, rnbo = oracle_ops.group(x, rcen, ri)
    assert torch.equal(cen.cpu(), rcen)
    assert torch.equal(nb.cpu(), rnb) and torch.equal(nbo.cpu(), rnbo)


def test_b128_bf16_graph_replay_equals_eager_and_fp32_band():
    from gm3d_amd import engine_pretrain as E
    steps = 6
    pool = [clouds.uniform(B, 1024, 150 + i).cuda() for i in range(3)]
    noise = [torch.rand(B, 64, generator=torch.Generator().manual_seed(i)).cuda() for i in range(steps + 3)]
    keys = ("loss_chfr", "loss_learn", "grad_norm")

    m, ema, opt = _build()
    eager, masks = [], []
    for i in range(steps + 3):
        o = E.pretrain_step(m, ema, opt, pool[i % 3].clone(), 200, _args(True), mask_noise=noise[i], augment=False)
        eager.append([float(o[k]) for k in keys])
        masks.append(o["mask"].clone())
    for mk in masks:
        assert mk.dtype == torch.bool and mk.shape == (B, 64) and bool((mk.sum(dim=1) == 39).all())
    p_eager = opt.P.clone()
    del m, ema, opt

    m, ema, opt = _build()
    for i in range(3):      # the same three eager iterations, then capture without further warm-up
        E.pretrain_step(m, ema, opt, pool[i % 3].clone(), 200, _args(True), mask_noise=noise[i], augment=False)
    g = E.GraphedPretrainStep(m, ema, opt, _args(True), pool[0], 200, warmup_iters=0, augment=False, inject_mask_noise=True)
    got = []
    for i in range(3, steps + 3):
        o = g(pool[i % 3], noise[i])
        torch.cuda.synchronize()
        got.append([float(o[k]) for k in keys])
        assert torch.equal(o["mask"], masks[i])                 # same teacher, same noise: identical masks
    # replay == eager, EXACTLY: every kernel of the step is deterministic (own kernels with fixed-order reductions; the index
    # gathers' backward scatters over permutations, i.e. without colliding atomics) and a captured launch runs the same code on
    # the same operands (tools/eager_vs_graph_diag.py: flat gradient buffer bit-identical eager vs captured, B = 4 and 32)
    assert got == eager[3:], (got, eager[3:])
    assert torch.equal(opt.P, p_eager), float((opt.P - p_eager).abs().max())
    del g, m, ema, opt

    # fp32 eager step on the first batch: the bf16 losses of step 0 within the bf16 band (8 mantissa bits through 16 blocks)
    m, ema, opt = _build(flat=False)
    o = E.pretrain_step(m, ema, opt, pool[0].clone(), 200, _args(False), mask_noise=noise[0], augment=False)
    f32 = [float(o[k]) for k in keys]
    assert abs(eager[0][0] - f32[0]) <= 3e-2 * abs(f32[0]), (eager[0], f32)       # Chamfer loss
    assert abs(eager[0][1] - f32[1]) <= 5e-2 * abs(f32[1]), (eager[0], f32)       # ranking loss (sign decisions on near-ties)


MULT = 3.0              # bar = MULT x the reference's own bf16-autocast error at this size (tests/golden/pretrain_bf16.npz, b128/)
NOISE_REL, NOISE_FLOOR = 1e-5, 1e-4     # analytically-zero gradients: see tests/test_gpu_bf16_parity.py
# epoch 200: a cloud whose fp32 9th/10th-highest loss_pred gap is below GAP_MARGIN x the expected bf16 error of one loss_pred element
# (the reference's autocast rel-L2 x the RMS of loss_pred; a swap then needs two elements ~2.8 sigma apart) may pick another top 9
# and is excluded.  The det-filled teacher's loss_pred sits close together: 76 of the 128 clouds are excluded (measured), hence
GAP_MARGIN = 4.0
MAX_EXCLUDED = 0.65


def _build_det(bf16):
    """det-filled (the weights pretrain_bf16.npz's b128 errors were measured with), DropPath off; bf16: the flat optimizer the
    bench step uses (its gradient buffer opt.G is what the update reads)."""
    from gm3d_amd import engine_pretrain as E, models_mae_learn_loss as M
    from oracle import model_ref as R
    torch.manual_seed(0)
    m = M.mae_vit_base_patch16_dec512d8b(norm_pix_loss=False)
    R.det_fill_(m, seed=0)
    m = m.cuda().train()
    for mod in m.modules():
        if isinstance(mod, M.DropPath):
            mod.drop_prob = 0.0
    ema = E.ModelEma(m, 0.999)
    opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema) if bf16 else E.build_optimizer(m, lr=2e-4)
    return m, ema, opt


def test_b128_bf16_every_gradient_against_fp32():
    """All 251 gradients of the bf16 step (flat gradient buffer, by name) against the fp32 eager step on identical inputs and
    noise, at epoch 0 (the mask is the noise ranking: identical in both by construction); teacher loss_pred and the student's
    loss matrix too.  Then the guided mask at epoch 200: equal wherever the fp32 teacher's top-9 set is not a near-tie."""
    import numpy as np
    from gm3d_amd import engine_pretrain as E
    from tests.golden.make_golden_bf16 import B128_CLOUD_SEED, B128_NOISE_SEED
    from tests.parity import Ledger
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "pretrain_bf16.npz"))
    names = [str(n) for n in gold["param_names"]]
    x = clouds.uniform(B, 1024, B128_CLOUD_SEED).cuda()
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(B128_NOISE_SEED)).cuda()
    want = torch.ones(B, 64, dtype=torch.bool)
    want.scatter_(1, torch.argsort(noise.cpu(), dim=1)[:, :25], False)          # epoch 0: the 25 lowest-noise tokens stay visible
    res = {}
    for bf16 in (True, False):
        m, ema, opt = _build_det(bf16)
        o = E.step_forward_backward(m, ema, x.clone(), 0, _args(bf16), mask_noise=noise, augment=False, optimizer=opt)
        if bf16:
            opt.gather_grads()
            grads = {n: opt.G[o_: o_ + p.numel()].view_as(p).detach().cpu().double() for (n, p), o_ in zip(opt._named, opt._offs)}
        else:
            grads = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters() if p.grad is not None}
        o200 = E.step_forward_backward(m, ema, x.clone(), 200, _args(bf16), mask_noise=noise, augment=False, optimizer=opt)
        torch.cuda.synchronize()
        res[bf16] = dict(grads=grads, mask=o["mask"].cpu(), lp=o["teacher_loss_pred"].float().cpu(), matrix=o["matrix"].float().cpu(),
                         mask200=o200["mask"].cpu(), lp200=o200["teacher_loss_pred"].float().cpu())
        del m, ema, opt, o, o200
    b, f = res[True], res[False]
    assert torch.equal(b["mask"], f["mask"]) and torch.equal(f["mask"], want)
    assert sorted(f["grads"]) == sorted(names) and sorted(b["grads"]) == sorted(names)

    led = Ledger("B=128 bf16 vs fp32 (bar = %.0f x the reference's autocast error)" % MULT)
    for k in ("lp", "matrix"):
        ac = float(gold["b128/ac_err::" + {"lp": "teacher_loss_pred", "matrix": "matrix"}[k]])
        led.rel(k, b[k], f[k], MULT * ac)
        led.cos(k, b[k], f[k], 0.999)
        led.tiles(k, b[k], f[k], "act", floor=1e-3 * float(f[k].abs().max()))
    norms = gold["b128/gradnorm_all"]
    total = float(np.sqrt((norms ** 2).sum()))
    f_total = sum(float(g.pow(2).sum()) for g in f["grads"].values()) ** 0.5
    for n, g_ref, a in zip(names, norms, gold["b128/ac_abs_grad"]):
        bar = MULT * float(a) * f_total / total          # the reference's absolute error, at this model's gradient scale
        if float(g_ref) <= NOISE_REL * total:
            bar = max(bar, NOISE_FLOOR * f_total)
        err = float((b["grads"][n] - f["grads"][n]).norm())
        led.add("grad " + n, err, bar)
        if b["grads"][n].dim() >= 2 and float(g_ref) > NOISE_REL * total:
            led.tiles("grad " + n, b["grads"][n], f["grads"][n], "weight", floor=1e-3 * float(f["grads"][n].abs().max()))
    print(led.report(12))
    led.assert_ok()

    # epoch 200: the top len_loss = 9 predicted-loss tokens are always masked, the rest by the (shared) noise ranking
    assert torch.equal(b["lp200"], b["lp"]) and torch.equal(f["lp200"], f["lp"])        # same teacher, same input
    top = f["lp"].sort(dim=1, descending=True).values
    gap = top[:, 8] - top[:, 9]
    err_one = float(gold["b128/ac_err::teacher_loss_pred"]) * float(f["lp"].pow(2).mean().sqrt())
    clear = gap > GAP_MARGIN * err_one
    differ = (b["mask200"] != f["mask200"]).any(dim=1)
    n_ex = int((~clear).sum())
    print("epoch 200: %d of %d clouds excluded as near-ties (gap <= %.3g); %d masks differ overall" % (n_ex, B, GAP_MARGIN * err_one,
                                                                                                      int(differ.sum())))
    assert not bool((differ & clear).any()), "bf16 mask differs on clear clouds %s" % (differ & clear).nonzero().flatten().tolist()
    assert n_ex <= MAX_EXCLUDED * B, (n_ex, B)
    assert bool((b["mask200"].sum(dim=1) == 39).all())

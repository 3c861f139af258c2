"""-m gpu: soft targets for the classification fine-tune -- gm3d_soft_ce_fwd / _bwd and gm3d_mixup_points (gm3d_amd/csrc/soft_ce.hip)
through gm3d_amd/losses.py, and their wiring in engine_finetune / point_m2ae_cls.

  * loss, row losses and gradient against an fp64 restatement, at every shape where the kernels change their walk (one class, one
    row, rows shorter / exactly / longer than a wave, the longest row, more rows than the forward's 16 waves and than its mean's 64
    lanes), in the three target forms, f32 and bf16 logits, logits scaled by 1 and by 80;
  * out-of-range labels, the C-ABI refusals, the mixing launch against the aten expression bit for bit;
  * a captured loss node follows new coefficients; captured fine-tune steps with smoothing (+ mixup) equal eager ones bit for bit;
  * the default path launches what the parent commit launched; no result depends on unwritten memory."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import clouds

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (5, 15), (4, 40), (3, 63), (3, 64), (3, 65), (2, 1024), (257, 40)]
COEF = (0.55, 0.3, 0.004)          # (wa, wb, u): rows that do not sum to 1
DLOSS = 0.37


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _case(B, C, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, C, generator=g) * scale).to(dtype).cuda()
    ya = torch.randint(0, C, (B,), generator=g).cuda()
    yb = torch.randint(0, C, (B,), generator=g).cuda()
    yb[0] = ya[0]                                              # one row with ya == yb
    dense = (torch.rand(B, C, generator=g) * 0.7).cuda()       # rows that do not sum to 1
    return z, ya, yb, dense


def _dense_of(form, C, ya, yb, dense, coef):
    """the target rows of a form as fp64, from the f32 coefficients the kernel reads"""
    if form == "dense":
        return dense.double()
    wa, wb, u = (float(v) for v in coef.cpu())
    t = torch.full((ya.numel(), C), u, dtype=torch.float64, device=ya.device)
    t[torch.arange(ya.numel()), ya] += wa
    if form == "compact2":
        t[torch.arange(ya.numel()), yb] += wb
    return t


def _restate(z, t, dloss):
    """row_i = sum_c t_ic (lse_i - z_ic), loss = mean_i row_i, dlogits = dloss / B (S_i exp(z - lse_i) - t) in z's precision"""
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    row = (t * (lse - z)).sum(1)
    dz = dloss / z.size(0) * (t.sum(1, keepdim=True) * torch.exp(z - lse) - t)
    return row.mean(), row, dz


def _aten32(z, t, dloss):
    """the fp32 chain a user would write: timm's sum(-t * log_softmax(x), -1).mean() and autograd"""
    z = z.float().clone().requires_grad_(True)
    row = torch.sum(-t.float() * F.log_softmax(z, dim=-1), dim=-1)
    loss = row.mean()
    (loss * dloss).backward()
    return loss.detach(), row.detach(), z.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_loss_and_gradient_against_fp64(B, C, dtype):
    """Bar (tests/test_gpu_m2ae_cls.py's for this head): within 1e-5 of the fp64 restatement relative to its largest element, or within
    3x the distance of the fp32 aten restatement from fp64 where fp32 cannot do better.  bf16 logits: the restatement runs on the
    bf16-rounded logits; loss and row losses are f32 and held to the same bar; dlogits is rounded once to bf16, so each element may
    additionally be half a bf16 ulp (8 bits of precision: at most 2^-8 of its own size) from the fp64 value."""
    from gm3d_amd import losses as L
    coef = torch.tensor(COEF, dtype=torch.float32).cuda()
    for scale in (1.0, 80.0):
        z, ya, yb, dense = _case(B, C, dtype, scale, seed=B * 1000 + C)
        for form in ("compact2", "compact1", "dense"):
            kw = {"compact2": dict(ya=ya, yb=yb, coef=coef), "compact1": dict(ya=ya, coef=coef), "dense": dict(dense=dense)}[form]
            loss, row, lse = L.soft_ce_forward(z, **kw)
            zk = z.clone().requires_grad_(True)
            lk = L.soft_cross_entropy(zk, **kw)
            assert lk.dtype == torch.float32 and lk.dim() == 0 and torch.equal(lk.detach(), loss)
            (lk * DLOSS).backward()
            assert zk.grad.dtype == dtype
            t = _dense_of(form, C, ya, yb, dense, coef)
            l64, r64, g64 = _restate(z.double(), t, DLOSS)
            l32, r32, g32 = _aten32(z, t, DLOSS)
            what = (B, C, str(dtype), scale, form)
            for name, k, a, d in (("loss", loss, l32, l64), ("row_loss", row, r32, r64), ("dlogits", zk.grad, g32, g64)):
                ek, ea = _rel(k, d), _rel(a, d)
                print(what, name, "kernel %.3e aten32 %.3e" % (ek, ea))
                bar = max(1e-5, 3.0 * ea)
                if name == "dlogits" and dtype == torch.bfloat16:
                    err = (k.double() - d).abs()
                    assert bool((err <= 2.0 ** -8 * d.abs() + bar * d.abs().max()).all()), (what, name, ek, ea)
                else:
                    assert ek <= bar, (what, name, ek, ea)


def test_an_out_of_range_label_makes_its_row_nan_and_leaves_the_others():
    from gm3d_amd import losses as L
    coef = torch.tensor(COEF, dtype=torch.float32).cuda()
    z, ya, yb, _ = _case(5, 15, torch.float32, 1.0, seed=7)
    _, row, _ = L.soft_ce_forward(z, ya=ya, yb=yb, coef=coef)
    zg = z.clone().requires_grad_(True)
    L.soft_cross_entropy(zg, ya=ya, yb=yb, coef=coef).backward()
    for which, bad in (("ya", 15), ("ya", -1), ("yb", 15)):
        a, b = ya.clone(), yb.clone()
        (a if which == "ya" else b)[2] = bad
        loss2, row2, _ = L.soft_ce_forward(z, ya=a, yb=b, coef=coef)
        keep = torch.tensor([0, 1, 3, 4]).cuda()
        assert bool(torch.isnan(row2[2])) and bool(torch.isnan(loss2))
        assert torch.equal(row2[keep], row[keep])
        z2 = z.clone().requires_grad_(True)
        L.soft_cross_entropy(z2, ya=a, yb=b, coef=coef).backward()
        assert bool(torch.isnan(z2.grad[2]).all()) and torch.equal(z2.grad[keep], zg.grad[keep])


def test_c_abi_refusals_return_their_codes_and_launch_nothing():
    from gm3d_amd import _capi, ops
    from gm3d_amd._capi import lib
    p, st = ops._ptr, ops._stream()

    def call(B, C, form):
        n = max(B, 1)
        z = torch.zeros(n, C).cuda()
        ya, yb, coef = torch.zeros(n, dtype=torch.long).cuda(), torch.zeros(n, dtype=torch.long).cuda(), torch.tensor(COEF).cuda()
        dense = torch.zeros(n, C).cuda()
        outs = [torch.full((n,), 7.0).cuda(), torch.full((n,), 7.0).cuda(), torch.full((1,), 7.0).cuda(), torch.full((n, C), 7.0).cuda()]
        comp = (p(ya), p(yb), p(coef)) if form in ("compact", "both") else (None, None, None)
        dn = p(dense) if form in ("dense", "both") else None
        rf = lib.gm3d_soft_ce_fwd(p(z), B, C, *comp, dn, p(outs[0]), p(outs[1]), p(outs[2]), _capi.GM3D_F32, st)
        rb = lib.gm3d_soft_ce_bwd(p(z), B, C, *comp, dn, p(outs[1]), p(outs[2]), p(outs[3]), _capi.GM3D_F32, st)
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs), (B, C, form)
        return rf, rb

    assert call(4097, 2, "compact") == (_capi.GM3D_EUNSUPPORTED,) * 2
    assert call(4097, 2, "dense") == (_capi.GM3D_EUNSUPPORTED,) * 2
    assert call(2, 1025, "compact") == (_capi.GM3D_EUNSUPPORTED,) * 2
    assert call(3, 5, "both") == (_capi.GM3D_EINVAL,) * 2
    assert call(3, 5, "neither") == (_capi.GM3D_EINVAL,) * 2
    assert call(0, 5, "compact") == (_capi.GM3D_OK,) * 2
    assert call(0, 5, "dense") == (_capi.GM3D_OK,) * 2
    z = torch.zeros(3, 5).cuda()
    o = torch.zeros(3).cuda()
    assert lib.gm3d_soft_ce_fwd(p(z), 3, 5, None, None, None, p(z), p(o), p(o), p(o), 7, st) == _capi.GM3D_EINVAL      # dtype code
    assert lib.gm3d_soft_ce_fwd(p(z), 3, 5, None, None, None, p(z), None, p(o), p(o), _capi.GM3D_F32, st) == _capi.GM3D_EINVAL
    # the mixing launch: out of place only, labels both or neither
    x, perm, c2 = torch.zeros(2, 4, 3).cuda(), torch.arange(2).cuda(), torch.tensor([1.0, 0.0]).cuda()
    y = torch.zeros(2, dtype=torch.long).cuda()
    out = torch.full((2, 4, 3), 7.0).cuda()
    assert lib.gm3d_mixup_points(p(x), 2, 4, p(perm), p(c2), p(y), p(x), p(y), st) == _capi.GM3D_EINVAL
    assert lib.gm3d_mixup_points(p(x), 2, 4, p(perm), p(c2), p(y), p(out), None, st) == _capi.GM3D_EINVAL
    assert lib.gm3d_mixup_points(p(x), 2, 0, p(perm), p(c2), None, p(out), None, st) == _capi.GM3D_EINVAL
    assert lib.gm3d_mixup_points(p(x), 0, 4, p(perm), p(c2), None, p(out), None, st) == _capi.GM3D_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("B,N", [(1, 1), (4, 33), (8, 1024)])
def test_mixing_launch_equals_the_aten_expression(B, N):
    from gm3d_amd import losses as L
    g = torch.Generator().manual_seed(B * 100 + N)
    x = torch.randn(B, N, 3, generator=g).cuda()
    ya = torch.randint(0, 40, (B,), generator=g).cuda()
    mix = L.PointMixup(0.2)
    shuffled = torch.randperm(B, generator=g)
    for lam, perm in ((0.37, shuffled), (1.0, shuffled), (0.0, shuffled), (0.37, torch.arange(B))):
        mix.draw(B, "cuda", lam=lam, perm=perm)
        out, tgt = mix.mix(x, ya)
        dp = perm.cuda()
        assert torch.equal(out, lam * x + (1 - lam) * x[dp]), (lam, perm)
        assert torch.equal(tgt.ya, ya) and torch.equal(tgt.yb, ya[dp]) and tgt.lam == lam
        assert out.data_ptr() != x.data_ptr()


def test_a_captured_loss_node_follows_new_coefficients():
    from gm3d_amd import losses as L
    from gm3d_amd import streams
    z, ya, yb, _ = _case(32, 40, torch.float32, 1.0, seed=5)
    z.requires_grad_(True)
    coef = torch.tensor(COEF, dtype=torch.float32).cuda()

    def node():
        loss = L.soft_cross_entropy(z, ya=ya, yb=yb, coef=coef)
        return loss, torch.autograd.grad(loss * DLOSS, z)[0]

    streams.warm_up(node, 2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with streams.capture(graph):
        gl, gg = node()
    seen = []
    for lam in (1.0, 0.25, 0.0):
        coef.copy_(torch.from_numpy(L.LabelSmoothingCrossEntropy(0.1).coefficients(40, lam)))
        graph.replay()
        rl, rg = gl.clone(), gg.clone()
        el, eg = node()
        assert torch.equal(rl, el) and torch.equal(rg, eg), lam
        seen.append(float(rl))
    assert len(set(seen)) == 3 and all(np.isfinite(seen))


# --------------------------------------------------------------------------- the engine
def _steps(make_model, make_crit, graphed, bf16, batches, targets, with_mixup):
    """three warm-up iterations on batches[0] with the first draws, then one iteration per batch with fresh draws -- eagerly, or as
    GraphedFinetuneStep does it (tests/test_gpu_finetune.py::test_graph_replay_equals_eager's scheme)"""
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import losses as L
    args = SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=0, epochs=300)
    m = make_model()
    m.train()
    crit = make_crit(m)
    opt = EF.build_optimizer(m, lr=1e-3, capturable=True, flat=True, max_norm=10.0)
    EF.adjust_learning_rate(opt, 5.0, args)
    rng = np.random.RandomState(7)
    mix = L.PointMixup(0.2, rng=np.random.RandomState(11), generator=torch.Generator().manual_seed(12)) if with_mixup else None
    B = batches[0].size(0)
    if graphed:
        g = EF.GraphedFinetuneStep(m, crit, opt, batches[0], targets, npoints=1024, max_norm=10.0, bf16=bf16, rng=rng, augment=False,
                                   warmup_iters=3, mixup=mix)
        step = lambda x: g(x, targets)
    else:
        sub = rng.choice(1200, 1024, False)
        if mix is not None:
            mix.draw(B, "cuda")
        for _ in range(3):
            EF.finetune_step(m, crit, opt, batches[0], targets, npoints=1024, max_norm=10.0, bf16=bf16, subset=sub, augment=False,
                             mixup=mix, mixup_drawn=True)
        # the subset is drawn while the arguments are evaluated, the mixup inside the step: subset, lam, permutation
        step = lambda x: EF.finetune_step(m, crit, opt, x, targets, npoints=1024, max_norm=10.0, bf16=bf16,
                                          subset=rng.choice(1200, 1024, False), augment=False, mixup=mix)
    losses, lams = [], []
    for x in batches:
        losses.append(step(x)["loss"].clone())
        lams.append(None if mix is None else mix.lam)
    torch.cuda.synchronize()
    return losses, lams, {k: v.detach().clone() for k, v in m.named_parameters()}


def _batches():
    return [clouds.gaussian(8, 2048, seed=50 + i).cuda() for i in range(3)], (torch.arange(8).cuda() * 3) % 40


def test_point_transformer_step_with_mixup_and_smoothing_replay_equals_eager():
    from gm3d_amd import losses as L
    from tests.test_gpu_finetune import build
    batches, targets = _batches()
    make = lambda: build(seed=9, drop_path=0.0)
    crit = lambda m: L.LabelSmoothingCrossEntropy(0.1)
    le, lame, pe = _steps(make, crit, False, False, batches, targets, True)
    lg, lamg, pg = _steps(make, crit, True, False, batches, targets, True)
    assert lame == lamg and len(set(lame)) == 3                 # the same host draws, a new one per step
    assert all(torch.equal(a, b) for a, b in zip(le, lg)), ([float(v) for v in le], [float(v) for v in lg])
    assert all(torch.equal(pg[k], pe[k]) for k in pe)
    assert all(np.isfinite(float(v)) for v in le)
    # and the soft targets are in the loss: the same steps without them end elsewhere
    lp, _, _ = _steps(make, lambda m: nn.CrossEntropyLoss(), False, False, batches, targets, False)
    assert not torch.equal(lp[0], le[0])


def test_m2ae_classifier_step_with_smooth_replay_equals_eager():
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import losses as L
    from tests.test_gpu_m2ae_cls import MODELNET, _classifier
    batches, targets = _batches()
    made = []

    def make():
        m = _classifier(dict(MODELNET, smooth=0.3), seed=9)[1].cuda()
        made.append(m)
        return m
    le, _, pe = _steps(make, EF.build_criterion, False, True, batches, targets, False)
    lg, _, pg = _steps(make, EF.build_criterion, True, True, batches, targets, False)
    assert all(isinstance(m.loss_ce, L.SmoothLoss) and isinstance(EF.build_criterion(m), L.SmoothLoss) for m in made)
    assert all(torch.equal(a, b) for a, b in zip(le, lg)), ([float(v) for v in le], [float(v) for v in lg])
    assert all(torch.equal(pg[k], pe[k]) for k in pe)
    assert all(np.isfinite(float(v)) for v in le)


# one eager fine-tune step (PointTransformer of tests/test_gpu_finetune.py, B = 8, 2048 points, bf16, flat optimizer, plain cross-entropy):
# the names ops._launch was given and how often, as a KernelTimer records them.  Recorded on the parent commit of the soft-target change.
PARENT_LAUNCHES = [
    ["gm3d_fps", 2], ["gm3d_gather_points", 1], ["gm3d_knn_group", 1], ["gm3d_moments3", 1], ["gm3d_colsum_finish_f64", 3],
    ["gm3d_pn1_finalize", 1], ["gm3d_pn_layer1_fwd", 1], ["gm3d_gemm_tn_bf16_dma_pool", 2], ["gm3d_gemm_tn_bf16_dmaw", 5],
    ["gm3d_bn_bcast_stats", 1], ["gm3d_colsum_finish", 6], ["gm3d_bn_finalize", 1], ["gm3d_bn_bcast_apply_relu", 1],
    ["gm3d_lin3_gelu_fwd", 1], ["gm3d_residual_ln_fwd", 25], ["gm3d_gemm_tn_bf16_ring", 75], ["gm3d_attention_fwd", 12],
    ["gm3d_gemm_tn_bf16_dma_gelu", 12], ["gm3d_transpose_bf16_multi", 1], ["gm3d_residual_ln_bwd", 25],
    ["gm3d_gemm_tn_bf16_dma_gelu_bwd", 12], ["gm3d_attention_bwd", 12], ["gm3d_colsum_finish_batched", 2], ["gm3d_gemm_nt_bf16", 1],
    ["gm3d_colsum_partial", 3], ["gm3d_transpose_bf16_batched", 4], ["gm3d_lin3_gelu_bwd", 1], ["gm3d_group_max_bwd", 1],
    ["gm3d_bn_bcast_bwd_stats", 1], ["gm3d_bn_bcast_bwd_apply", 1], ["gm3d_group_scatter_add", 1], ["gm3d_pn_layer1_bwd_stats", 1],
    ["gm3d_pn1_bwd_finalize", 1], ["gm3d_gemm_nt_bf16_multi", 1], ["gm3d_adamw_ema_flat_step", 1]]
NEW_KERNELS = ("gm3d_soft_ce_fwd", "gm3d_soft_ce_bwd", "gm3d_mixup_points")


def _recorded_step(crit, mixup):
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    from tests.test_gpu_finetune import build
    pm = build(seed=9, drop_path=0.0)
    pm.train()
    opt = EF.build_optimizer(pm, lr=1e-3, flat=True, max_norm=10.0)
    pts = clouds.gaussian(8, 2048, seed=50).cuda()
    targets = (torch.arange(8).cuda() * 3) % 40
    sub = np.random.RandomState(7).choice(1200, 1024, False)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        EF.finetune_step(pm, crit, opt, pts, targets, npoints=1024, max_norm=10.0, subset=sub, mixup=mixup)
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    return [[n, len(r)] for n, r in timer.records.items()]


def test_the_default_step_launches_what_the_parent_commit_launched():
    from gm3d_amd import losses as L
    got = _recorded_step(nn.CrossEntropyLoss(), None)
    assert got == PARENT_LAUNCHES
    assert not any(n in NEW_KERNELS for n, _ in got)
    # switched on, the three launches join the same list once each and nothing else changes
    soft = _recorded_step(L.LabelSmoothingCrossEntropy(0.1), L.PointMixup(0.2, rng=np.random.RandomState(1)))
    assert sorted(map(tuple, soft)) == sorted(map(tuple, PARENT_LAUNCHES + [[n, 1] for n in NEW_KERNELS]))


@pytest.mark.parametrize("pattern", ["nan", "+inf", "-inf"])
def test_no_result_depends_on_unwritten_memory(pattern):
    """Every allocation of gm3d_amd/losses.py filled with NaN / +inf / -inf (tests/poison.py) before a kernel writes it: losses, row
    losses, lse, gradients, mixed clouds and labels are the same bits as without.  engine_finetune.py gained no allocation.  The sites
    stay recorded in poison.SITES: they count as reached for the coverage condition of the poison modules, which run after this one."""
    from gm3d_amd import losses as L
    from tests import poison
    coef = torch.tensor(COEF, dtype=torch.float32).cuda()
    z, ya, yb, dense = _case(5, 15, torch.float32, 1.0, seed=3)
    zb = z.to(torch.bfloat16)
    x = clouds.gaussian(4, 33, seed=4).cuda()
    lab = torch.tensor([3, 1, 4, 1]).cuda()
    mix = L.PointMixup(0.2)
    mix.draw(4, "cuda", lam=0.37, perm=torch.tensor([2, 0, 3, 1]))

    def run():
        out = []
        for logits in (z, zb):
            for kw in (dict(ya=ya, yb=yb, coef=coef), dict(ya=ya, coef=coef), dict(dense=dense)):
                out.extend(L.soft_ce_forward(logits, **kw))
                zz = logits.clone().requires_grad_(True)
                loss = L.soft_cross_entropy(zz, **kw)
                (loss * DLOSS).backward()
                out.extend([loss.detach(), zz.grad])
        crit = L.SmoothLoss(0.3)
        mixed, tgt = mix.mix(x, lab)
        out.extend([mixed, tgt.ya, tgt.yb, crit(z[:4], tgt).detach(), crit(z, ya).detach()])
        torch.cuda.synchronize()
        return out

    want = run()
    with poison.poisoned(pattern) as ps:
        got = run()
    sites = poison.scan_sites()
    mine = {s for s in sites if s.startswith("gm3d_amd/losses.py:")}
    assert len(mine) == 6 and mine <= ps.sites, sorted(mine - ps.sites)
    new_in_engine = {s for s in sites if s.startswith("gm3d_amd/engine_finetune.py:")}
    assert len(new_in_engine) == 1, new_in_engine               # validate_vote's `vt`, from before: the step allocates nothing itself
    poison.assert_same(want, got, "soft_targets")

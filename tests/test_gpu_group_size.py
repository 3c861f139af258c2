"""-m gpu: patches of 8 and 16 points.  The fused masked-patch loss for k = 8 / 16 (csrc/chamfer.hip patch_loss_small_*) against the
op chain it replaces, on ties and under poison; GeoMask3D at 128 x 16 and 256 x 8 against the CPU oracle, captured against eager, and
its reconstruction pass; plain Point-MAE against the fixture the reference's own model made at its config_2 / config_3 geometries
(tests/golden/point_mae_pretrain_groups.npz); and the default 64 x 32 step, whose loss launches are the ones it always made.

This module runs before tests/test_gpu_poison_ops.py / _steps.py (alphabetical order): the allocation lines it reaches under poison
stay recorded in poison.SITES and count for their coverage condition."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from tests import clouds
from tests import point_mae_ref as PR
from tests import poison
from tests.test_gpu_model import FeedDropPath, rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LOSS_LAUNCHES = ("gm3d_patch_chamfer_loss_fwd", "gm3d_patch_chamfer_loss_bwd", "gm3d_patch_chamfer_l1_loss_fwd",
                 "gm3d_patch_chamfer_l1_loss_bwd", "gm3d_patch_chamfer_loss_k_fwd", "gm3d_patch_chamfer_loss_k_bwd",
                 "gm3d_patch_chamfer_l1_loss_k_fwd", "gm3d_patch_chamfer_l1_loss_k_bwd", "gm3d_chamfer_fwd", "gm3d_chamfer_bwd")


def _timed(fn):
    """-> (fn(), {launch name: count}) with an ops.KernelTimer installed around the call"""
    from gm3d_amd import ops
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.set_kernel_timer(None)
    return out, {n: len(r) for n, r in timer.records.items()}


def _loss_launches(counts):
    return {n: c for n, c in counts.items() if n in LOSS_LAUNCHES}


# ----------------------------------------------------------------------------------------------------------------- the fused loss
def _loss_inputs(B, M, k, dtype, lattice=False):
    """pix (B,L,3k) with L = M + 5, target (B,L,k,3), a (B,L) permutation buffer: pred and mask_ids are their last-M slices"""
    L = M + 5
    g = torch.Generator().manual_seed(B * 1000 + M * 10 + k)
    if lattice:          # four values per coordinate: equal distances abound
        pix = torch.randint(0, 4, (B, L, 3 * k), generator=g).float() * 0.25
        target = torch.randint(0, 4, (B, L, k, 3), generator=g).float() * 0.25
    else:
        pix, target = torch.randn(B, L, 3 * k, generator=g) * 0.3, torch.randn(B, L, k, 3, generator=g) * 0.3
    order = torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).cuda()
    return pix.cuda().to(dtype).requires_grad_(True), target.cuda(), order, L


def _fused(pix, target, order, M, l1, full=False):
    """-> (mean, matrix, idx1, idx2, d mean * 3 / d pix) through the fused function, on the batch-strided slices"""
    from gm3d_amd import heads
    L = pix.shape[1]
    mask_ids, pred = order[:, L - M:], pix[:, L - M:]
    assert heads.patch_chamfer_loss_supported(pred, target, mask_ids)
    assert not pred.is_contiguous() and not mask_ids.is_contiguous()
    if full:
        mean, matrix = heads.PatchChamferLossFn.apply(pix, target, mask_ids, True)
    else:
        mean, matrix = (heads.PatchChamferL1LossFn if l1 else heads.PatchChamferLossFn).apply(pred, target, mask_ids)
    i1, i2 = mean.grad_fn.saved_tensors[3:5]
    pix.grad = None
    (mean * 3.0).backward()
    grad, pix.grad = pix.grad, None
    return mean.detach(), matrix, i1, i2, grad


def _chain(pix, target, order, M, k, l1):
    """the op chain forward_loss / _patch_loss run without the fused kernel: gather, cast, ops.chamfer, the means, autograd"""
    from gm3d_amd import models_mae_learn_loss as M_
    from gm3d_amd import ops
    B, L = order.shape
    tg = M_.take(target, order[:, L - M:]).reshape(-1, k, 3)
    p32 = pix[:, L - M:].reshape(-1, k, 3).to(torch.float32)
    d1, d2, i1, i2 = ops.chamfer(p32.detach().contiguous(), tg)
    if l1:
        mean = ops.ChamferDistanceL1()(p32, tg)
        matrix = ((d1.sqrt().mean(1) + d2.sqrt().mean(1)) / 2).reshape(B, M)
    else:
        matrix = ops.ChamferDistanceL2()(p32, tg).reshape(B, -1, k).mean(dim=-1)
        mean = matrix.mean()
    pix.grad = None
    (mean * 3.0).backward()
    grad, pix.grad = pix.grad, None
    return mean.detach(), matrix.detach(), i1, i2, grad


@pytest.mark.parametrize("l1", [False, True], ids=["cdl2", "cdl1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,M", [(3, 1), (5, 13), (4, 77), (2, 154)])
@pytest.mark.parametrize("k", [8, 16])
def test_small_patch_loss_equals_the_op_chain(k, B, M, dtype, l1):
    """B * M = 3, 65, 308, 308 patches on segments of k lanes: never a multiple of the 256 / k patches of a workgroup, the last one
    mostly dead.  Argmins equal ops.chamfer's on the gathered patches; matrix, mean and dpred within the bars of
    tests/test_gpu_heads.py::test_patch_chamfer_loss_equals_the_op_chain (2e-6 relative; a bf16 dpred 2^-8 of its maximum): every
    summed term is non-negative, so the error of a sum of n terms is below n * 2^-24 of it -- n = 2k - 1 <= 31 for a patch, far inside.
    full=True (cdl2): zeros for the lead rows, the rest the sliced call's bits."""
    pix, target, order, L = _loss_inputs(B, M, k, dtype)
    mean, matrix, i1, i2, grad = _fused(pix, target, order, M, l1)
    want_mean, want_matrix, w1, w2, want_grad = _chain(pix, target, order, M, k, l1)
    assert tuple(i1.shape) == (B * M, k) and i1.dtype == torch.int32 and tuple(matrix.shape) == (B, M)
    assert torch.equal(i1, w1) and torch.equal(i2, w2)
    em = float((matrix - want_matrix).abs().max()) / float(want_matrix.abs().max())
    es = abs(float(mean) - float(want_mean)) / abs(float(want_mean))
    scale = float(want_grad.float().abs().max())
    eg = float((grad.float() - want_grad.float()).abs().max()) / scale
    tol = 2e-6 if dtype == torch.float32 else 2.0 ** -8
    print("k %d B %d M %d %s %s: matrix %.3e mean %.3e (2e-6), dpred %.3e (%.1e)" % (k, B, M, dtype, "cdl1" if l1 else "cdl2", em, es, eg, tol))
    assert em <= 2e-6 and es <= 2e-6
    assert grad.dtype == dtype and tuple(grad.shape) == (B, L, 3 * k)
    assert eg <= tol
    assert float(grad[:, :L - M].abs().max()) == 0.0
    if not l1:
        fmean, fmatrix, f1, f2, fgrad = _fused(pix, target, order, M, False, full=True)
        assert torch.equal(fmean, mean) and torch.equal(fmatrix, matrix) and torch.equal(f1, i1) and torch.equal(f2, i2)
        assert bool((fgrad[:, :L - M] == 0).all()) and torch.equal(fgrad, grad)


@pytest.mark.parametrize("k", [8, 16])
def test_small_patch_loss_on_ties(k):
    """Predictions and targets on a lattice of four values per coordinate: most points have several nearest neighbours at exactly the
    same distance.  The argmins are still ops.chamfer's in both directions (first minimum: j == 0 seeds, strict <, ascending j), for
    cdl2 and cdl1.  The f32 cdl2 gradient EQUALS the chain's (torch.equal): chamfer_small_bwd_kernel sums a predicted point's slot in
    the same order (its own term, then the reverse-direction terms in ascending j) with the same weight (g / (B M)) / k, so no
    tolerance is needed.  (cdl1's gradient is not defined on this input: coincident points give inf * 0.)"""
    B, M = 5, 13
    pix, target, order, L = _loss_inputs(B, M, k, torch.float32, lattice=True)
    mean, matrix, i1, i2, grad = _fused(pix, target, order, M, False)
    want_mean, want_matrix, w1, w2, want_grad = _chain(pix, target, order, M, k, False)
    tg = target.gather(1, order[:, L - M:].reshape(B, M, 1, 1).expand(B, M, k, 3)).reshape(-1, k, 3)
    d = (pix.detach()[:, L - M:].reshape(-1, k, 1, 3) - tg.reshape(-1, 1, k, 3)).pow(2).sum(-1)
    tied = (d == d.min(dim=2, keepdim=True).values).sum(dim=2) > 1
    assert float(tied.float().mean()) > 0.2          # the input does what it is for (0.28 of the points at k = 8, 0.44 at 16)
    assert torch.equal(i1, w1) and torch.equal(i2, w2)
    assert float((matrix - want_matrix).abs().max()) <= 2e-6 * float(want_matrix.abs().max())
    assert abs(float(mean) - float(want_mean)) <= 2e-6 * abs(float(want_mean))
    assert bool((want_grad != 0).any()) and torch.equal(grad, want_grad)
    from gm3d_amd import heads
    lmean, _ = heads.PatchChamferL1LossFn.apply(pix[:, L - M:], target, order[:, L - M:])
    l1, l2 = lmean.grad_fn.saved_tensors[3:5]
    assert torch.equal(l1, w1) and torch.equal(l2, w2)


@pytest.mark.parametrize("pattern", sorted(poison.PATTERNS))
def test_small_patch_launches_write_all_they_return(pattern):
    """every torch.empty behind the new launches filled with NaN / +inf / -inf first: matrix, mean, both argmin maps and dpred (sliced,
    full=True and cdl1; f32 and bf16) carry the bits of a plain run"""
    def run():
        out = {}
        for k in (8, 16):
            for dtype in (torch.float32, torch.bfloat16):
                for B, M in ((3, 1), (4, 77)):
                    pix, target, order, _ = _loss_inputs(B, M, k, dtype)
                    key = "k%d-%s-B%d-M%d" % (k, dtype, B, M)
                    out[key + "-cdl2"] = _fused(pix, target, order, M, False)
                    out[key + "-full"] = _fused(pix, target, order, M, False, full=True)
                    out[key + "-cdl1"] = _fused(pix, target, order, M, True)
        return out

    plain = run()
    with poison.poisoned(pattern) as state:
        pois = run()
    assert state.recorded > 0
    poison.assert_same(plain, pois, "small_patch_loss")


def test_other_patch_sizes_are_refused():
    from gm3d_amd import heads
    for k in (4, 12, 24, 64):
        pix = torch.zeros(2, 9, 3 * k, device="cuda")
        target = torch.zeros(2, 9, k, 3, device="cuda")
        ids = torch.arange(9, device="cuda").repeat(2, 1)
        assert not heads.patch_chamfer_loss_supported(pix, target, ids)
    pix, target = torch.zeros(2, 9, 48, device="cuda"), torch.zeros(2, 9, 8, 3, device="cuda")          # rows of 3 * 16, patches of 8
    assert not heads.patch_chamfer_loss_supported(pix, target, torch.arange(9, device="cuda").repeat(2, 1))


# ----------------------------------------------------------------------------------------------------------------- GeoMask3D vs the oracle
class _NoiseRng:
    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def shuffle(self, arr):
        n = self.noise[self.i][torch.from_numpy(arr)]
        arr[:] = arr[torch.argsort(n).numpy()]
        self.i += 1


def _mask_sizes(L, ratio, epoch, total=400):
    len_keep = int(L * (1 - ratio))
    return len_keep, int((L - len_keep) * (float((epoch + 1) / total) * 0.5))


def _geomask(G, k, seed, drop_path=0.0):
    from gm3d_amd import models_mae_learn_loss as M
    torch.manual_seed(0)
    pm = M.mae_vit_base_patch16_dec512d8b(num_group=G, group_size=k)
    for mod in pm.modules():
        if isinstance(mod, M.DropPath) and drop_path is not None:
            mod.drop_prob = drop_path
    return R.det_fill_(pm, seed=seed).cuda().train()


@pytest.mark.parametrize("G,k,B", [(128, 16, 4), (256, 8, 2)])
def test_step_against_oracle_at_other_group_sizes(G, k, B):
    """tests/test_gpu_geomask_groups.py::test_step_against_oracle_at_other_group_counts at 128 x 16 (B = 4) and 256 x 8 (B = 2), its
    body and its bars: fp32, DropPath off, mask noise injected, epoch 200 of 400.  Mask equality with the CPU oracle is a condition on
    the inputs: the ORACLE's teacher loss_pred has, in every cloud, a gap of at least 1e-4 of its range at the forced-set boundary
    (asserted below on the oracle's values alone; 2.7e-3 and 5.5e-4 with these seeds)."""
    from gm3d_amd import engine_pretrain as E
    torch.manual_seed(0)
    om = R.det_fill_(R.PointMAEGM3D(drop_path_rate=0.0, num_group=G, group_size=k), seed=3)
    pm = _geomask(G, k, seed=3)
    om.train()
    oema, pema = R.ModelEma(om, decay=0.999), E.ModelEma(pm, decay=0.999)
    oopt = torch.optim.AdamW(R.param_groups(om, 0.05), lr=1e-3)
    popt = E.build_optimizer(pm, lr=1e-3, weight_decay=0.05)
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=False, accum_iter=1)
    x = clouds.gaussian(B, 1024, seed=77)
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(9))
    pre = {n: v.detach().cpu().clone() for n, v in pm.named_parameters()}
    pre_ema = {n: v.detach().cpu().clone() for n, v in pema.ema.state_dict().items()}
    ores = R.pretrain_step(om, oema, oopt, x.clone(), epoch=200, total_epoch=400, mask_rng=_NoiseRng(noise))
    len_keep, len_loss = _mask_sizes(G, 0.6, 200)
    assert len_loss > 0
    s = ores["teacher_loss_pred"].sort(dim=1).values
    gap = (s[:, G - len_loss] - s[:, G - len_loss - 1]) / (s[:, -1] - s[:, 0])
    print("G %d k %d: forced-set gap %.3e of the range (needs 1e-4)" % (G, k, float(gap.min())))
    assert float(gap.min()) >= 1e-4, gap
    pres, counts = _timed(lambda: E.pretrain_step(pm, pema, popt, x.clone().cuda(), 200, args, mask_noise=noise, augment=False))
    assert _loss_launches(counts) == {"gm3d_patch_chamfer_loss_k_fwd": 1, "gm3d_patch_chamfer_loss_k_bwd": 1}
    assert torch.equal(pres["mask"].cpu(), ores["mask"])
    figs = (rel(pres["loss_chfr"], ores["chamfer"]), rel(pres["loss_learn"], ores["loss_learn"]), rel(pres["grad_norm"], ores["grad_norm"]))
    print("G %d k %d: chamfer rel %.3e (1e-5), loss_learn rel %.3e (1e-5), grad_norm rel %.3e (2e-5)" % ((G, k) + figs))
    assert figs[0] <= 1e-5
    assert figs[1] <= 1e-5
    assert figs[2] <= 2e-5
    # optimizer / EMA arithmetic on the product's own gradients through torch's AdamW on the CPU; the gradients against the oracle's
    cpu = {n: torch.nn.Parameter(v.clone()) for n, v in pre.items()}
    for n, p in pm.named_parameters():
        cpu[n].grad = p.grad.detach().cpu().clone()
    decay = [cpu[n] for n, p in pm.named_parameters() if not (p.dim() == 1 or n.endswith(".bias") or "token" in n)]
    nodecay = [cpu[n] for n, p in pm.named_parameters() if (p.dim() == 1 or n.endswith(".bias") or "token" in n)]
    torch.optim.AdamW([{"params": nodecay, "weight_decay": 0.0}, {"params": decay, "weight_decay": 0.05}], lr=1e-3).step()
    psd = dict(pm.named_parameters())
    assert max(rel(psd[n], cpu[n]) for n in cpu) <= 1e-6
    og = dict(om.named_parameters())
    worst = (0.0, None)
    for n, p in pm.named_parameters():
        err = float((p.grad.double().cpu() - og[n].grad.double()).abs().max())
        bar = 2e-4 * float(og[n].grad.abs().max()) + 1e-5 * float(ores["grad_norm"])
        worst = max(worst, (err / bar, n))
        assert err <= bar, (n, err, bar)
    print("G %d k %d: worst gradient tensor at %.3f of its bar (%s)" % (G, k, worst[0], worst[1]))
    pesd = pema.ema.state_dict()
    for n, v in pre_ema.items():
        if v.dtype.is_floating_point:
            src = psd[n].detach().cpu() if n in psd else pm.state_dict()[n].cpu()
            assert rel(pesd[n], v * 0.999 + 0.001 * src) <= 1e-6, n


# ----------------------------------------------------------------------------------------------------------------- captured step
def test_captured_step_at_128x16_replays_to_the_eager_trajectory():
    """128 x 16, bf16, B = 8: three replays of GraphedPretrainStep equal three eager steps from the same state -- the losses, the
    gradient norm, the flat parameter and EMA buffers, with torch.equal.  One eager step records the small-patch loss forward and
    backward once each and no gm3d_chamfer_fwd (the op chain), and issues no aten sort / scatter / topk."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    from tests.test_gpu_geomask_groups import _Ops
    G, k, B, steps = 128, 16, 8, 3
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
    pool = [clouds.uniform(B, 1024, 50 + i).cuda() for i in range(3)]
    noise = [torch.rand(B, G, generator=torch.Generator().manual_seed(i)).cuda() for i in range(steps + 3)]

    def build():
        torch.manual_seed(0)
        m = M.mae_vit_base_patch16_dec512d8b(num_group=G, group_size=k).cuda().train()
        for mod in m.modules():
            if isinstance(mod, M.DropPath):
                mod.drop_prob = 0.0
        ema = E.ModelEma(m, 0.999)
        return m, ema, E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema)

    def warm(m, ema, opt):
        for i in range(3):
            E.pretrain_step(m, ema, opt, pool[i % 3].clone(), 200, args, mask_noise=noise[i], augment=False)

    keys = ("loss_chfr", "loss_learn", "grad_norm")
    m, ema, opt = build()
    warm(m, ema, opt)
    eager = []
    for i in range(3, steps + 3):
        o = E.pretrain_step(m, ema, opt, pool[i % 3].clone(), 200, args, mask_noise=noise[i], augment=False)
        eager.append({n: o[n].clone() for n in keys} | {"P": opt.P.clone(), "E": opt.E.clone()})

    def one():
        with _Ops() as seen:
            E.pretrain_step(m, ema, opt, pool[0].clone(), 200, args, mask_noise=noise[0], augment=False)
        return seen
    ops_seen, counts = _timed(one)
    assert _loss_launches(counts) == {"gm3d_patch_chamfer_loss_k_fwd": 1, "gm3d_patch_chamfer_loss_k_bwd": 1}
    names = [n for n, _ in ops_seen.seen]
    assert len(names) > 50
    assert not [n for n in names if any(w in n for w in ("sort", "scatter", "topk"))], sorted(set(names))

    m, ema, opt = build()
    warm(m, ema, opt)
    g = E.GraphedPretrainStep(m, ema, opt, args, pool[0], 200, warmup_iters=0, augment=False, inject_mask_noise=True)
    for j, i in enumerate(range(3, steps + 3)):
        o = g(pool[i % 3], noise[i])
        torch.cuda.synchronize()
        for n in keys:
            assert bool(torch.isfinite(o[n])) and torch.equal(o[n], eager[j][n]), (i, n, float(o[n]), float(eager[j][n]))
        assert torch.equal(opt.P, eager[j]["P"]) and torch.equal(opt.E, eager[j]["E"]), i


# ----------------------------------------------------------------------------------------------------------------- plain Point-MAE
FX_CASES = (("g128k16_cdl2", 128, 16, 0.75, "cdl2"), ("g256k8_cdl2", 256, 8, 0.6, "cdl2"), ("g256k8_cdl1", 256, 8, 0.6, "cdl1"))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "point_mae_pretrain_groups.npz"))


def _point_mae(G, k, ratio, loss, seed=41, drop_path=None):
    from gm3d_amd import models_mae_learn_loss as MM
    from gm3d_amd.point_mae import Point_MAE
    cfg = PR.config("rand", loss, num_group=G, group_size=k)
    cfg["transformer_config"]["mask_ratio"] = ratio
    torch.manual_seed(0)
    m = R.det_fill_(Point_MAE(cfg), seed=seed)
    if drop_path is not None:
        for mod in m.modules():
            if isinstance(mod, MM.DropPath):
                mod.drop_prob = drop_path
    return m.cuda().train()


@pytest.mark.parametrize("case", FX_CASES, ids=[c[0] for c in FX_CASES])
def test_point_mae_fp32_parity_with_the_reference_fixture(fx, case, monkeypatch):
    """tests/test_gpu_point_mae_pretrain.py::test_fp32_parity_with_the_reference_fixture at the reference's config_2 (128 x 16, mask
    ratio 0.75) and config_3 (256 x 8, cdl2 and cdl1) geometries: the fixture's mask injected, its DropPath draws replayed; the loss and
    the six recorded gradients within 1e-5 relative.  The loss came from the fused small-patch launches, not the op chain."""
    from gm3d_amd import models_mae_learn_loss as M
    name, G, k, ratio, loss_type = case
    m = _point_mae(G, k, ratio, loss_type)
    pts = torch.from_numpy(fx["pts"]).cuda()
    mask = torch.from_numpy(fx[name + "/mask"]).cuda()
    feed = FeedDropPath(fx[name + "/droppath_masks"])
    monkeypatch.setattr(M, "drop_path", feed)
    monkeypatch.setattr(M, "drop_path_scale", feed.scale)

    def step():
        out = m(pts.clone(), mask=mask)
        out.backward()
        return out.detach()
    loss, counts = _timed(step)
    assert feed.masks == []
    stem = "gm3d_patch_chamfer_loss_k_" if loss_type == "cdl2" else "gm3d_patch_chamfer_l1_loss_k_"
    assert _loss_launches(counts) == {stem + "fwd": 1, stem + "bwd": 1}
    ref = float(fx[name + "/loss"])
    print(name, "loss", float(loss), "fixture", ref, "rel", abs(float(loss) - ref) / abs(ref))
    named = dict(m.named_parameters())
    stride = int(fx["stride"])
    errs = {}
    for key in PR.GRADS:
        errs[key] = rel(PR.picked(named[key].grad, stride), fx[name + "/grad/" + key])
        n = float(fx[name + "/gradnorm/" + key])
        print(name, key, "rel err", errs[key], "norm rel", abs(float(named[key].grad.double().norm()) - n) / n)
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    for key in PR.GRADS:
        assert errs[key] <= 1e-5, (key, errs[key])
        n = float(fx[name + "/gradnorm/" + key])
        assert abs(float(named[key].grad.double().norm()) - n) <= 1e-5 * n, key


def test_point_mae_replay_equals_eager_at_128x16():
    """GraphedPointMAEStep at 128 x 16 (B = 4, bf16) with injected draws against pretrain_step fed the same draws, three steps from
    identical state: loss, flat parameters and both moment buffers equal after every step."""
    from gm3d_amd import engine_pretrain_point_mae as EP
    from tests.test_gpu_point_mae_pretrain import _args
    G, B, steps = 128, 4, 3
    m = _point_mae(G, 16, 0.75, "cdl2", drop_path=0.0)
    opt = EP.build_optimizer(m)
    args = _args()
    x = [clouds.gaussian(B, 1024, seed=500 + i).cuda() for i in range(steps)]
    gen = torch.Generator().manual_seed(17)
    noise = [torch.rand(B, G, generator=gen).cuda() for _ in range(steps)]
    g = EP.GraphedPointMAEStep(m, opt, x[0], args, warmup_iters=2, augment=False, inject_mask_noise=True)
    state = ({n: v.clone() for n, v in m.state_dict().items()}, opt.M.clone(), opt.V.clone(), opt.step_dev.clone())

    def restore():
        with torch.no_grad():
            m.load_state_dict(state[0])
            opt.M.copy_(state[1]); opt.V.copy_(state[2]); opt.step_dev.copy_(state[3])
            opt.sync_shadows()
            if opt.GA is not None:
                opt.GA.zero_()

    restore()
    want = []
    for i in range(steps):
        (o, counts) = _timed(lambda: EP.pretrain_step(m, opt, x[i].clone(), args, mask_noise=noise[i], augment=False, micro_step=i))
        assert _loss_launches(counts) == {"gm3d_patch_chamfer_loss_k_fwd": 1, "gm3d_patch_chamfer_loss_k_bwd": 1}
        want.append((o["loss"].clone(), opt.P.clone(), opt.M.clone(), opt.V.clone()))
    restore()
    for i in range(steps):
        o = g(x[i], mask_noise=noise[i], update=True)
        got = (o["loss"], opt.P, opt.M, opt.V)
        assert bool(torch.isfinite(got[0]))
        assert all(torch.equal(a, b) for a, b in zip(got, want[i])), (i, float(got[0]), float(want[i][0]))
    assert not torch.equal(want[0][1], want[steps - 1][1])          # the parameters did move


# ----------------------------------------------------------------------------------------------------------------- reconstruction
def test_reconstruct_geomask_at_128x16():
    """tests/test_gpu_geomask_groups.py::test_reconstruct_geomask_at_128_groups with patches of 16 points: the mask and ids are the
    engine's sequence, the dense clouds the aten chain's bit for bit, patch_loss the fused loss's matrix"""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import reconstruct as RC
    from tests.test_gpu_point_mae_reconstruct import aten_chain
    G, K, B = 128, 16, 2
    m = _geomask(G, K, seed=0, drop_path=None)
    ema = E.ModelEma(m, 0.999)
    V = int(G * (1 - 0.6))
    NM = G - V
    pts = clouds.gaussian(B, 1024, seed=61).cuda()
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(2)).cuda()
    r, counts = _timed(lambda: RC.reconstruct_geomask(m, ema, pts, epoch=100, total_epoch=400, mask_ratio=0.6, mask_noise=noise))
    assert counts.get("gm3d_patch_chamfer_loss_k_fwd") == 1 and "gm3d_patch_chamfer_loss_fwd" not in counts
    assert m.training
    assert tuple(r.teacher_loss_pred.shape) == (B, G) and tuple(r.loss_pred.shape) == (B, NM) and tuple(r.pred.shape) == (B, NM, 3 * K)
    _, vis_ids, mask_ids, mask = M.generate_mask_ids(r.teacher_loss_pred, 0.6, True, 100, 400, noise, want_bool=True)
    assert torch.equal(r.mask, mask) and torch.equal(r.vis_ids, vis_ids) and torch.equal(r.mask_ids, mask_ids)
    assert int(mask.sum()) == B * NM
    m.eval()
    with torch.no_grad():
        outs = m(pts, mask=mask, num_visible=V, ids=(vis_ids, mask_ids))
        pred = outs["pix_pred"][:, -NM:]
        lo = m.forward_loss(pred, outs["neighborhood"], mask, mask_ids=mask_ids, full_pred=outs["pix_pred"])
    assert tuple(outs["pix_pred"].shape) == (B, G, 3 * K) and tuple(outs["neighborhood"].shape) == (B, G, K, 3)
    want_dense, want_fc = aten_chain(pred, outs["neighborhood"], outs["center"], vis_ids, mask_ids, False)
    assert torch.equal(r.dense, want_dense.view(B, G * K, 3)) and torch.equal(r.center, want_fc.view(B, G, 3))
    assert torch.equal(r.patch_loss, lo["matrix"]) and torch.equal(r.loss, lo["Chamfer_mean"])
    assert torch.equal(r.loss_pred, outs["loss_pred"][:, -NM:].float())
    assert r.n_visible == V * K and bool(torch.isfinite(r.cd_l2).all()) and bool(torch.isfinite(r.cd_l1).all())


def test_point_mae_vis_at_256x8_and_reconstruct_at_128x16(fx):
    """Point_MAE(vis=True) at 256 x 8 and reconstruct.reconstruct at 128 x 16, on the fixture's clouds and masks: the dense clouds and
    centre lists are the aten chain's (P/models/Point_MAE.py:429-437) on the model's own prediction, bit for bit"""
    from gm3d_amd import reconstruct as RC
    from tests.test_gpu_point_mae_reconstruct import aten_chain
    pts = torch.from_numpy(fx["pts"]).cuda()
    B = pts.shape[0]
    G, K = 256, 8
    m = _point_mae(G, K, 0.6, "cdl2").eval()
    mask = torch.from_numpy(fx["g256k8_cdl2/mask"]).cuda()
    V = G - int(0.6 * G)
    with torch.no_grad():
        ret1, ret2, full_center = m(pts.clone(), vis=True, mask=mask)
        neighborhood, center, _ = m.group_divider(pts.clone())
        _, vis_ids, mask_ids, pred, _ = m._rebuild(neighborhood, center, mask=mask)
    assert tuple(ret1.shape) == (1, B * G * K, 3) and tuple(ret2.shape) == (1, B * V * K, 3) and tuple(full_center.shape) == (B * G, 3)
    want_dense, want_fc = aten_chain(pred, neighborhood, center, vis_ids, mask_ids, True)
    assert torch.equal(ret1[0], want_dense) and torch.equal(full_center, want_fc) and torch.equal(ret2[0], want_dense[:B * V * K])

    G, K = 128, 16
    m = _point_mae(G, K, 0.75, "cdl2").eval()
    mask = torch.from_numpy(fx["g128k16_cdl2/mask"]).cuda()
    r, counts = _timed(lambda: RC.reconstruct(m, pts, mask=mask))
    assert counts.get("gm3d_patch_chamfer_loss_k_fwd") == 1
    with torch.no_grad():
        neighborhood, center, _ = m.group_divider(pts.clone())
        _, vis_ids, mask_ids, pred, _ = m._rebuild(neighborhood, center, mask=mask, chosen=True)
        loss, matrix = m._patch_loss(pred, neighborhood, mask_ids, True)
    want_dense, want_fc = aten_chain(pred, neighborhood, center, vis_ids, mask_ids, False)
    assert torch.equal(r.dense, want_dense.view(B, G * K, 3)) and torch.equal(r.center, want_fc.view(B, G, 3))
    assert torch.equal(r.patch_loss, matrix) and torch.equal(r.loss, loss) and r.n_visible == (G - 96) * K
    assert abs(float(r.patch_loss.mean()) - float(r.loss)) <= 1e-5 * abs(float(r.loss))


# ----------------------------------------------------------------------------------------------------------------- the default size
def test_default_size_launches_what_it_always_launched():
    """64 x 32: one eager fp32 step records gm3d_patch_chamfer_loss_fwd and _bwd once each, as on the commit before group_size, and
    none of the k-sized names; forward_loss equals PatchChamferLossFn called directly on the same tensors, bit for bit."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import heads
    from gm3d_amd import models_mae_learn_loss as M
    G, B = 64, 2
    pm = _geomask(G, 32, seed=1)
    assert pm.group_size == 32 and M.mae_vit_base_patch16_dec512d8b().group_size == 32
    ema = E.ModelEma(pm, decay=0.999)
    opt = E.build_optimizer(pm, lr=1e-3, weight_decay=0.05)
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=False, accum_iter=1)
    x = clouds.uniform(B, 1024, seed=42).cuda()
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(1))
    _, counts = _timed(lambda: E.pretrain_step(pm, ema, opt, x.clone(), 0, args, mask_noise=noise, augment=False))
    assert _loss_launches(counts) == {"gm3d_patch_chamfer_loss_fwd": 1, "gm3d_patch_chamfer_loss_bwd": 1}
    assert not [n for n in counts if "_k_" in n]
    pm.eval()
    V = int(G * (1 - 0.6))
    with torch.no_grad():
        lp = torch.randn(B, G, generator=torch.Generator().manual_seed(3)).cuda()
        _, vis_ids, mask_ids, mask = M.generate_mask_ids(lp, 0.6, True, 0, 400, noise.cuda(), want_bool=True)
        outs = pm(x, mask=mask, num_visible=V, ids=(vis_ids, mask_ids))
        pred = outs["pix_pred"][:, -(G - V):]
        lo = pm.forward_loss(pred, outs["neighborhood"], mask, mask_ids=mask_ids, full_pred=outs["pix_pred"])
        mean, matrix = heads.PatchChamferLossFn.apply(pred, outs["neighborhood"], mask_ids)
    assert torch.equal(lo["Chamfer_mean"], mean) and torch.equal(lo["matrix"], matrix) and bool(torch.isfinite(mean))

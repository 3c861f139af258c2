"""-m gpu: GeoMask3D Point-MAE at group counts other than 64.  The guided mask (gm3d_mask_select) and the pairwise ranking loss
(gm3d_rank_loss / gm3d_rank_loss_tail) for 65..512 tokens per cloud (csrc/guided.hip) against their CPU formulations, then the whole
step against the oracle, the captured step against the eager one, reconstruct_geomask, and the launches' outputs under poison."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from oracle import model_ref as R
from tests import clouds
from tests import poison
from tests.test_gpu_model import rel

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------- guided mask
def _mask_sizes(L, ratio, epoch, total=400):
    len_keep = int(L * (1 - ratio))
    return len_keep, int((L - len_keep) * (float((epoch + 1) / total) * 0.5))


def _argsort_mask(lp, noise, ratio, epoch):
    """generate_mask (P/:744-784) with stable sorts + split_ids on the CPU: the formulation of tests/test_gpu_heads.py"""
    from gm3d_amd import models_mae_learn_loss as M
    B, L = lp.shape
    len_keep, len_loss = _mask_sizes(L, ratio, epoch)
    nz = noise.clone()
    if len_loss > 0:
        forced = torch.argsort(lp, dim=1, stable=True)[:, L - len_loss:]
        nz.scatter_(1, forced, float("inf"))
    keep = torch.argsort(nz, dim=1, stable=True)[:, :len_keep]
    want = torch.ones(B, L)
    want.scatter_(1, keep, 0.0)
    wv, wm = M.split_ids(want.bool(), len_keep)
    return want, wv, wm


def _mask_inputs(B, L, ties):
    g = torch.Generator().manual_seed(B * 1000 + L)
    lp, noise = torch.randn(B, L, generator=g), torch.rand(B, L, generator=g)
    if ties:                             # heavy ties: halves and eighths
        lp, noise = (lp * 2).round() / 2, (noise * 8).floor() / 8
    return lp, noise


MASK_CASES = [(L, 0.6, e, False) for L in (65, 128, 200, 512) for e in (0, 200, 399)] + [(200, 0.6, 200, True), (512, 0.6, 399, True),
                                                                                           (65, 0.0, 200, False)]


@pytest.mark.parametrize("L,ratio,epoch,ties", MASK_CASES)
def test_guided_mask_equals_stable_argsort(L, ratio, epoch, ties):
    from gm3d_amd import models_mae_learn_loss as M
    B = 3
    lp, noise = _mask_inputs(B, L, ties)
    want, wv, wm = _argsort_mask(lp, noise, ratio, epoch)
    mask, vis, msk, mb = M.generate_mask_ids(lp.cuda(), ratio, True, epoch, 400, noise.cuda(), want_bool=True)
    assert torch.equal(mask.cpu(), want) and torch.equal(mb.cpu(), want.bool())
    assert vis.shape == wv.shape and msk.shape == wm.shape
    assert torch.equal(vis.cpu(), wv) and torch.equal(msk.cpu(), wm)
    m = M.mae_vit_base_patch16_dec512d8b(num_group=L)
    assert torch.equal(m.generate_mask(lp.cuda(), ratio, epoch=epoch, total_epoch=400, noise=noise).cpu(), want)


def test_guided_mask_above_512_takes_the_fallback():
    """L = 513: the C entry point refuses it and generate_mask runs the aten formulation, with the same result"""
    from gm3d_amd import models_mae_learn_loss as M
    B, L, ratio, epoch = 3, 513, 0.6, 200
    lp, noise = _mask_inputs(B, L, False)
    want, wv, wm = _argsort_mask(lp, noise, ratio, epoch)
    m = M.mae_vit_base_patch16_dec512d8b()
    got = m.generate_mask(lp.cuda(), ratio, epoch=epoch, total_epoch=400, noise=noise)
    assert torch.equal(got.cpu(), want)
    gv, gm = M.split_ids(got.bool(), int(L * (1 - ratio)))
    assert torch.equal(gv.cpu(), wv) and torch.equal(gm.cpu(), wm)
    with pytest.raises(RuntimeError):
        M.generate_mask_ids(lp.cuda(), ratio, True, epoch, 400, noise.cuda())


@pytest.mark.parametrize("pitched", [True, False])
def test_guided_mask_with_nan_and_inf_stays_inside_its_rows(pitched):
    """L = 200, loss_pred and noise sprinkled with NaN (both signs), +inf, -inf and -0, one cloud all NaN: exactly len_keep tokens are
    visible, [vis | masked] is a permutation of 0..L-1 per row, and the NaN-filled bands around every output buffer are untouched."""
    from gm3d_amd._capi import check, lib
    from gm3d_amd.ops import _ptr, _stream
    B, L, guard = 4, 200, 256
    len_keep, len_loss = _mask_sizes(L, 0.6, 399)
    g = torch.Generator().manual_seed(5)
    lp, noise = torch.randn(B, L, generator=g), torch.rand(B, L, generator=g)
    special = [float("nan"), -float("nan"), float("inf"), -float("inf"), -0.0, 0.0]
    for t in (lp, noise):
        where = torch.randint(0, L, (B, 60), generator=g)
        what = torch.tensor(special)[torch.randint(0, len(special), (B, 60), generator=g)]
        t.scatter_(1, where, what)
    lp[2] = float("nan")
    noise[3] = float("inf")
    lp, noise = lp.cuda(), noise.cuda()
    nan32 = lambda n: torch.full((n,), float("nan"), device="cuda")
    mask = nan32(B * L + 2 * guard)
    mask_b = torch.full((B * L + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    pv, pm = (L, L) if pitched else (len_keep, L - len_keep)
    if pitched:       # the halves of one (B,L) order buffer
        order = torch.full((B * L + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda").view(torch.int64)
        vis_ptr, msk_ptr = order.data_ptr() + 8 * guard, order.data_ptr() + 8 * (guard + len_keep)
    else:             # two dense arrays
        vbuf = torch.full((B * pv + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda").view(torch.int64)
        mbuf = torch.full((B * pm + 2 * guard,), float("nan"), dtype=torch.float64, device="cuda").view(torch.int64)
        vis_ptr, msk_ptr = vbuf.data_ptr() + 8 * guard, mbuf.data_ptr() + 8 * guard
    nan64 = int(torch.full((1,), float("nan"), dtype=torch.float64).view(torch.int64))
    check(lib.gm3d_mask_select_b(_ptr(lp), _ptr(noise), B, L, len_keep, len_loss, ctypes.c_void_p(mask.data_ptr() + 4 * guard),
                                 ctypes.c_void_p(mask_b.data_ptr() + guard), ctypes.c_void_p(vis_ptr), ctypes.c_void_p(msk_ptr),
                                 L if pitched else 0, _stream()), "gm3d_mask_select")
    torch.cuda.synchronize()
    for buf in (mask[:guard], mask[-guard:]):
        assert bool(buf.isnan().all())
    assert bool((mask_b[:guard] == 0xA5).all()) and bool((mask_b[-guard:] == 0xA5).all())
    if pitched:
        assert bool((order[:guard] == nan64).all()) and bool((order[-guard:] == nan64).all())
        o = order[guard:-guard].view(B, L)
        vis, msk = o[:, :len_keep], o[:, len_keep:]
    else:
        for buf in (vbuf, mbuf):
            assert bool((buf[:guard] == nan64).all()) and bool((buf[-guard:] == nan64).all())
        vis, msk = vbuf[guard:-guard].view(B, pv), mbuf[guard:-guard].view(B, pm)
    m = mask[guard:-guard].view(B, L)
    assert bool(((m == 0) | (m == 1)).all())
    assert torch.equal((m == 0).sum(dim=1).cpu(), torch.full((B,), len_keep))
    assert torch.equal(mask_b[guard:-guard].view(B, L), (m == 1).to(torch.uint8))
    perm = torch.cat([vis, msk], dim=1)
    assert torch.equal(perm.sort(dim=1).values.cpu(), torch.arange(L).expand(B, L))
    assert bool((torch.gather(m, 1, vis) == 0).all()) and bool((torch.gather(m, 1, msk) == 1).all())
    assert bool((vis[:, 1:] > vis[:, :-1]).all()) and bool((msk[:, 1:] > msk[:, :-1]).all())      # each list ascending


# ----------------------------------------------------------------------------------------------------------------- ranking loss
RANK_CASES = [(3, 65), (1, 100), (3, 308), (2, 512)]
_rank_ref = {}


def _rank_case(B, M):
    """inputs (one pair of tied targets per row) and the fp64 expression of forward_learning_loss (P/:795-805) with its gradient, on the
    CPU; computed once per shape and shared"""
    if (B, M) not in _rank_ref:
        g = torch.Generator().manual_seed(B * 1000 + M)
        p, t = torch.randn(B, M, generator=g), torch.rand(B, M, generator=g)
        for b in range(B):
            t[b, 5 + b] = t[b, M - 7 - b]
        pd, td = p.double().requires_grad_(True), t.double()
        pos, neg = td.unsqueeze(1) > td.unsqueeze(2), td.unsqueeze(1) < td.unsqueeze(2)
        sig = torch.sigmoid(pd.unsqueeze(1) - pd.unsqueeze(2))
        loss = (-pos.double() * torch.log(sig + 1e-6) - neg.double() * torch.log(1 - sig + 1e-6)).sum() / (pos | neg).sum()
        (loss * 3.0).backward()
        _rank_ref[(B, M)] = (p, t, loss.detach(), pd.grad.clone())
    return _rank_ref[(B, M)]


def _check_rank(name, loss, grad, want_loss, want_grad):
    el = abs(float(loss) - float(want_loss)) / abs(float(want_loss))
    eg = float((grad.double().cpu() - want_grad).abs().max()) / float(want_grad.abs().max())
    print("%s: loss rel %.3e (bar 1e-5), grad / max %.3e (bar 2e-5)" % (name, el, eg))
    assert el <= 1e-5 and eg <= 2e-5, (name, el, eg)


@pytest.mark.parametrize("B,M", RANK_CASES)
def test_rank_loss_matches_fp64(B, M):
    from gm3d_amd import heads
    p, t, want_loss, want_grad = _rank_case(B, M)
    pc = p.cuda().requires_grad_(True)
    loss = heads.rank_loss(pc, t.cuda())
    (loss * 3.0).backward()
    _check_rank("rank_loss B%d M%d" % (B, M), loss, pc.grad, want_loss, want_grad)


@pytest.mark.parametrize("front", [0, 204])
@pytest.mark.parametrize("B,M", RANK_CASES)
def test_rank_loss_tail_matches_fp64(B, M, front):
    """the ranking loss on the last M of L = M + front columns; the gradient of the columns in front is zero"""
    from gm3d_amd import heads
    p, t, want_loss, want_grad = _rank_case(B, M)
    g = torch.Generator().manual_seed(front + 1)
    full = torch.cat([torch.randn(B, front, generator=g), p], dim=1).cuda().requires_grad_(True)
    loss = heads.rank_loss_tail(full, M, t.cuda())
    assert "_RankLossTail" in type(loss.grad_fn).__name__
    (loss * 3.0).backward()
    assert full.grad.shape == (B, M + front)
    assert bool((full.grad[:, :front] == 0).all())
    _check_rank("rank_loss_tail B%d M%d front %d" % (B, M, front), loss, full.grad[:, front:], want_loss, want_grad)


def test_rank_loss_of_constant_targets_is_nan():
    from gm3d_amd import heads
    p = torch.randn(2, 200, generator=torch.Generator().manual_seed(1)).cuda()
    t = torch.ones(2, 200).cuda()
    assert torch.isnan(heads.rank_loss(p, t))                    # 0 / 0 like the reference
    assert torch.isnan(heads.rank_loss_tail(p, 200, t))
    assert torch.isnan(heads.rank_loss_tail(p, 120, t[:, :120].contiguous()))


def test_forward_learning_loss_routes_wide_rows_to_the_kernels():
    """forward_learning_loss at M = 308 runs the launches (no (B,M,M) aten chain): its graph ends in the fused functions"""
    from gm3d_amd import models_mae_learn_loss as M
    p, t, want_loss, _ = _rank_case(3, 308)
    m = M.MaskedAutoencoderViT.__new__(M.MaskedAutoencoderViT)
    pc = p.cuda().requires_grad_(True)
    a = M.MaskedAutoencoderViT.forward_learning_loss(m, pc, None, t.cuda(), relative=True)
    b = M.MaskedAutoencoderViT.forward_learning_loss(m, pc, None, t.cuda(), relative=True, full_pred=pc)
    assert "_RankLoss" in type(a.grad_fn).__name__ and "_RankLossTail" in type(b.grad_fn).__name__
    assert rel(a, want_loss) <= 1e-5 and rel(b, want_loss) <= 1e-5


# ----------------------------------------------------------------------------------------------------------------- one step vs the oracle
class _NoiseRng:
    def __init__(self, noise):
        self.noise, self.i = noise, 0

    def shuffle(self, arr):
        n = self.noise[self.i][torch.from_numpy(arr)]
        arr[:] = arr[torch.argsort(n).numpy()]
        self.i += 1


@pytest.mark.parametrize("G,B", [(128, 4), (192, 2)])
def test_step_against_oracle_at_other_group_counts(G, B):
    """tests/test_gpu_model.py::test_step_against_oracle at num_group 128 (B = 4) and 192 (B = 2), with that test's bars: fp32, DropPath
    off, mask noise injected.  128: guided mask of two waves, 77 masked tokens on the wide ranking loss, the teacher's 128 tokens at the
    upper edge of the LDS attention, the student's 51 visible tokens; 192: 116 masked, the teacher on the flash attention, 76 visible.
    Mask equality with the CPU oracle is a condition on the inputs: the seeds are chosen so that the ORACLE's teacher loss_pred has, in
    every cloud, a gap of at least 1e-4 of its range at the forced-set boundary (asserted below on the oracle's values alone)."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    torch.manual_seed(0)
    om = R.det_fill_(R.PointMAEGM3D(drop_path_rate=0.0, num_group=G), seed=3)
    pm = M.mae_vit_base_patch16_dec512d8b(num_group=G)
    for mod in pm.modules():
        if isinstance(mod, M.DropPath):
            mod.drop_prob = 0.0
    R.det_fill_(pm, seed=3)
    pm = pm.cuda()
    om.train(); pm.train()
    oema, pema = R.ModelEma(om, decay=0.999), E.ModelEma(pm, decay=0.999)
    oopt = torch.optim.AdamW(R.param_groups(om, 0.05), lr=1e-3)
    popt = E.build_optimizer(pm, lr=1e-3, weight_decay=0.05)
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=False, accum_iter=1)
    x = clouds.gaussian(B, 1024, seed=77)
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(9))
    pre = {k: v.detach().cpu().clone() for k, v in pm.named_parameters()}
    pre_ema = {k: v.detach().cpu().clone() for k, v in pema.ema.state_dict().items()}
    ores = R.pretrain_step(om, oema, oopt, x.clone(), epoch=200, total_epoch=400, mask_rng=_NoiseRng(noise))
    # the condition on the inputs, on the oracle's values alone
    len_keep, len_loss = _mask_sizes(G, 0.6, 200)
    assert len_loss > 0 and G - len_keep > 64
    s = ores["teacher_loss_pred"].sort(dim=1).values
    gap = (s[:, G - len_loss] - s[:, G - len_loss - 1]) / (s[:, -1] - s[:, 0])
    assert float(gap.min()) >= 1e-4, gap
    pres = E.pretrain_step(pm, pema, popt, x.clone().cuda(), 200, args, mask_noise=noise, augment=False)
    assert torch.equal(pres["mask"].cpu(), ores["mask"])
    figs = (rel(pres["loss_chfr"], ores["chamfer"]), rel(pres["loss_learn"], ores["loss_learn"]), rel(pres["grad_norm"], ores["grad_norm"]))
    print("G %d: chamfer rel %.3e (1e-5), loss_learn rel %.3e (1e-5), grad_norm rel %.3e (2e-5)" % ((G,) + figs))
    assert figs[0] <= 1e-5
    assert figs[1] <= 1e-5
    assert figs[2] <= 2e-5
    # optimizer / EMA arithmetic on the product's own gradients through torch's AdamW on the CPU; the gradients against the oracle's
    cpu = {k: torch.nn.Parameter(v.clone()) for k, v in pre.items()}
    for k, p in pm.named_parameters():
        cpu[k].grad = p.grad.detach().cpu().clone()
    decay = [cpu[k] for k, p in pm.named_parameters() if not (p.dim() == 1 or k.endswith(".bias") or "token" in k)]
    nodecay = [cpu[k] for k, p in pm.named_parameters() if (p.dim() == 1 or k.endswith(".bias") or "token" in k)]
    torch.optim.AdamW([{"params": nodecay, "weight_decay": 0.0}, {"params": decay, "weight_decay": 0.05}], lr=1e-3).step()
    psd = dict(pm.named_parameters())
    assert max(rel(psd[k], cpu[k]) for k in cpu) <= 1e-6
    og = dict(om.named_parameters())
    worst = (0.0, None)
    for k, p in pm.named_parameters():
        err = float((p.grad.double().cpu() - og[k].grad.double()).abs().max())
        bar = 2e-4 * float(og[k].grad.abs().max()) + 1e-5 * float(ores["grad_norm"])
        worst = max(worst, (err / bar, k))
        assert err <= bar, (k, err, bar)
    print("G %d: worst gradient tensor at %.3f of its bar (%s)" % (G, worst[0], worst[1]))
    pesd = pema.ema.state_dict()
    for k, v in pre_ema.items():
        if v.dtype.is_floating_point:
            src = psd[k].detach().cpu() if k in psd else pm.state_dict()[k].cpu()
            assert rel(pesd[k], v * 0.999 + 0.001 * src) <= 1e-6, k


# ----------------------------------------------------------------------------------------------------------------- captured step
class _Ops(TorchDispatchMode):
    """the aten ops one step issues, with the largest tensor each read: (name, elements)"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        n = max([a.numel() for a in args if torch.is_tensor(a)] + [0])
        self.seen.append((str(func), n))
        return func(*args, **(kwargs or {}))


def test_captured_step_at_192_groups_replays_to_the_eager_trajectory():
    """num_group = 192, bf16, B = 8: three replays of GraphedPretrainStep equal three eager steps from the same state -- the losses, the
    gradient norm, the flat parameter and EMA buffers, with torch.equal.  That equality needs every reduction of the step in a fixed
    order: an eager step issues no aten sort / argsort / scatter (the guided mask) and no aten reduction over 32768 elements or more
    (aten's reductions go multi-block from about 64k; the (B,M,M) ranking-loss chain would be 8 * 116 * 116 = 107648)."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    G, B, steps = 192, 8, 3
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
    pool = [clouds.uniform(B, 1024, 50 + i).cuda() for i in range(3)]
    noise = [torch.rand(B, G, generator=torch.Generator().manual_seed(i)).cuda() for i in range(steps + 3)]

    def build():
        torch.manual_seed(0)
        m = M.mae_vit_base_patch16_dec512d8b(num_group=G).cuda().train()
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
        eager.append({k: o[k].clone() for k in keys} | {"P": opt.P.clone(), "E": opt.E.clone()})
    with _Ops() as ops_seen:
        E.pretrain_step(m, ema, opt, pool[0].clone(), 200, args, mask_noise=noise[0], augment=False)
    names = [n for n, _ in ops_seen.seen]
    assert len(names) > 50
    assert not [n for n in names if any(w in n for w in ("sort", "scatter", "topk"))], sorted(set(names))
    big = [(n, e) for n, e in ops_seen.seen if any(w in n for w in ("aten.sum", "aten.mean", "aten.norm", "aten.linalg_vector_norm",
                                                                   "aten.amax", "aten.max", "aten.var", "aten.prod")) and e >= 32768]
    assert not big, big

    m, ema, opt = build()
    warm(m, ema, opt)
    g = E.GraphedPretrainStep(m, ema, opt, args, pool[0], 200, warmup_iters=0, augment=False, inject_mask_noise=True)
    for j, i in enumerate(range(3, steps + 3)):
        o = g(pool[i % 3], noise[i])
        torch.cuda.synchronize()
        for k in keys:
            assert bool(torch.isfinite(o[k])) and torch.equal(o[k], eager[j][k]), (i, k, float(o[k]), float(eager[j][k]))
        assert torch.equal(opt.P, eager[j]["P"]) and torch.equal(opt.E, eager[j]["E"]), i


# ----------------------------------------------------------------------------------------------------------------- reconstruct_geomask
def test_reconstruct_geomask_at_128_groups():
    """tests/test_gpu_point_mae_reconstruct.py::test_reconstruct_geomask at num_group = 128: the mask and ids are the engine's sequence
    (generate_mask_ids on the teacher's predicted loss and the same noise) and the argsort formulation's, the dense clouds the aten
    chain's bit for bit"""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import reconstruct as RC
    from tests.test_gpu_point_mae_reconstruct import aten_chain
    G, K, B = 128, 32, 2
    torch.manual_seed(0)
    m = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(num_group=G), seed=0).cuda().train()
    ema = E.ModelEma(m, 0.999)
    V = int(G * (1 - 0.6))
    NM = G - V
    pts = clouds.gaussian(B, 1024, seed=61).cuda()
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(2)).cuda()
    r = RC.reconstruct_geomask(m, ema, pts, epoch=100, total_epoch=400, mask_ratio=0.6, mask_noise=noise)
    assert m.training
    assert tuple(r.teacher_loss_pred.shape) == (B, G) and tuple(r.loss_pred.shape) == (B, NM)
    _, vis_ids, mask_ids, mask = M.generate_mask_ids(r.teacher_loss_pred, 0.6, True, 100, 400, noise, want_bool=True)
    assert torch.equal(r.mask, mask) and torch.equal(r.vis_ids, vis_ids) and torch.equal(r.mask_ids, mask_ids)
    want, wv, wm = _argsort_mask(r.teacher_loss_pred.float().cpu(), noise.cpu(), 0.6, 100)
    assert torch.equal(mask.cpu(), want.bool()) and torch.equal(vis_ids.cpu(), wv) and torch.equal(mask_ids.cpu(), wm)
    assert int(mask.sum()) == B * NM
    m.eval()
    with torch.no_grad():
        outs = m(pts, mask=mask, num_visible=V, ids=(vis_ids, mask_ids))
        pred = outs["pix_pred"][:, -NM:]
        lo = m.forward_loss(pred, outs["neighborhood"], mask, mask_ids=mask_ids, full_pred=outs["pix_pred"])
    want_dense, want_fc = aten_chain(pred, outs["neighborhood"], outs["center"], vis_ids, mask_ids, False)
    assert torch.equal(r.dense, want_dense.view(B, G * K, 3)) and torch.equal(r.center, want_fc.view(B, G, 3))
    assert torch.equal(r.patch_loss, lo["matrix"]) and torch.equal(r.loss, lo["Chamfer_mean"])
    assert torch.equal(r.loss_pred, outs["loss_pred"][:, -NM:].float())
    assert r.n_visible == V * K and bool(torch.isfinite(r.cd_l2).all()) and bool(torch.isfinite(r.cd_l1).all())


# ----------------------------------------------------------------------------------------------------------------- poison
@pytest.mark.parametrize("pattern", sorted(poison.PATTERNS))
def test_wide_launches_write_all_they_return(pattern):
    """every torch.empty behind the wide launches filled with NaN / +inf / -inf first: the bits of the results are those of a plain run"""
    from gm3d_amd import heads
    from gm3d_amd import models_mae_learn_loss as M

    def run():
        out = {}
        for L, epoch in ((65, 0), (128, 200), (200, 399), (512, 200)):
            lp, noise = _mask_inputs(3, L, L == 200)
            out["mask%d" % L] = M.generate_mask_ids(lp.cuda(), 0.6, True, epoch, 400, noise.cuda(), want_bool=True)
        for B, Mm in RANK_CASES:
            p, t, _, _ = _rank_case(B, Mm)
            for front in (0, 204):
                g = torch.Generator().manual_seed(front + 1)
                full = torch.cat([torch.randn(B, front, generator=g), p], dim=1).cuda().requires_grad_(True)
                a = heads.rank_loss_tail(full, Mm, t.cuda())
                (a * 1.7).backward()
                out["tail%d-%d-%d" % (B, Mm, front)] = (a.detach(), full.grad)
            pc = p.cuda().requires_grad_(True)
            b = heads.rank_loss(pc, t.cuda())
            (b * 1.7).backward()
            out["plain%d-%d" % (B, Mm)] = (b.detach(), pc.grad)
        return out

    plain = run()
    with poison.poisoned(pattern) as state:
        pois = run()
    assert state.recorded > 0
    poison.assert_same(plain, pois, "wide")


# ----------------------------------------------------------------------------------------------------------------- 257..512 tokens, bf16
@pytest.mark.parametrize("T", [257, 400, 481, 512])
def test_stack_attention_between_the_lds_and_the_streaming_lengths(T):
    """bf16, head_dim 64: the LDS-resident attention holds 480 tokens forward and 256 backward and the streaming kernels start at 513;
    the stacks run the lengths in between on the streaming kernels at 513 rows with the padding blocked as keys (attention.fwd / bwd with
    pad=True).  Against softmax(Q K^T / 8) V in fp64 with the project's bf16 attention bars (tests/test_gpu_abi_edges.py: output
    2e-2, gradient 3e-2 of the reference's maximum); the forward below 481 is the LDS kernel's as before."""
    from gm3d_amd import attention
    B, H, hd = 2, 6, 64
    g = torch.Generator(device="cuda").manual_seed(T)
    qkv = torch.randn(B * T, 3 * H * hd, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(B * T, H * hd, device="cuda", generator=g).to(torch.bfloat16)
    out, lse = attention.fwd(qkv, None, B, T, H, hd, hd ** -0.5, head=True, pad=True)
    assert tuple(lse.shape) == (B, H, T if T <= 480 else attention.PAD_T)
    dqkv = attention.bwd(qkv, None, out, dout, lse, B, T, H, hd, hd ** -0.5, head=True, pad=True)
    q64 = qkv.double().requires_grad_(True)
    q, k, v = q64.view(B, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v).transpose(1, 2).reshape(B * T, H * hd)
    ref.backward(dout.double())
    eo, eg = rel(out, ref), rel(dqkv, q64.grad)
    print("T %d: out %.3e (bar 2e-2), dqkv %.3e (bar 3e-2)" % (T, eo, eg))
    assert tuple(out.shape) == (B * T, H * hd) and tuple(dqkv.shape) == tuple(qkv.shape)
    assert eo <= 2e-2 and eg <= 3e-2


def test_bf16_step_at_512_groups_is_close_to_fp32():
    """tests/test_gpu_model.py::test_bf16_step_runs_and_is_close at num_group = 512 (B = 2): the teacher and the decoders see 512 tokens
    (forward and backward on the padded streaming attention in bf16), the student 204, the guided mask and the ranking loss (M = 308)
    their widest rows.  Epoch 0: no token is forced, so both runs draw the same mask from the injected noise."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    G, B = 512, 2
    res = {}
    for bf16 in (False, True):
        torch.manual_seed(0)
        pm = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(num_group=G), seed=1).cuda().train()
        for mod in pm.modules():
            if isinstance(mod, M.DropPath):
                mod.drop_prob = 0.0
        ema = E.ModelEma(pm, decay=0.999)
        opt = E.build_optimizer(pm)
        args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=bf16, accum_iter=1)
        noise = torch.rand(B, G, generator=torch.Generator().manual_seed(2))
        out = E.pretrain_step(pm, ema, opt, clouds.uniform(B, 1024, 5).cuda(), 0, args, mask_noise=noise, augment=False)
        res[bf16] = (float(out["loss_chfr"]), float(out["loss_learn"]), float(out["grad_norm"]), out["mask"].clone())
        assert all(np.isfinite(v) for v in res[bf16][:3])
        assert int(out["mask"].sum()) == B * (G - int(G * 0.4))
    assert torch.equal(res[True][3], res[False][3])
    print("G 512: chamfer %.6f / %.6f, loss_learn %.6f / %.6f, grad_norm %.4f / %.4f (bf16 / fp32)" % (
        res[True][0], res[False][0], res[True][1], res[False][1], res[True][2], res[False][2]))
    assert abs(res[True][0] - res[False][0]) <= 3e-2 * abs(res[False][0])   # bf16: 8 significant bits per op
    assert abs(res[True][1] - res[False][1]) <= 3e-2 * abs(res[False][1])

"""-m gpu: plain Point-MAE pre-training -- the centre-masking kernel, the L1 patch loss, the model against the reference's fixture
(tests/golden/point_mae_pretrain_b4.npz), device masking against host ids, hipGraph replay against eager, the epoch engine and the
checkpoint as the published run's frozen teacher."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from tests import clouds
from tests import point_mae_ref as PR
from tests.test_gpu_model import FeedDropPath, rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "point_mae_pretrain_b4.npz"))


@pytest.fixture(scope="module")
def M():
    from gm3d_amd import models_mae_learn_loss as M
    return M


def _model(mask_type="rand", loss="cdl2", seed=41, drop_path=None, **kw):
    from gm3d_amd import models_mae_learn_loss as MM
    from gm3d_amd.point_mae import Point_MAE
    torch.manual_seed(0)
    m = R.det_fill_(Point_MAE(PR.config(mask_type, loss, **kw)), seed=seed)
    if drop_path is not None:
        for mod in m.modules():
            if isinstance(mod, MM.DropPath):
                mod.drop_prob = drop_path
    return m.cuda().train()


# --------------------------------------------------------------------------- gm3d_mask_centers
def _check_order(mask, order, G, num_mask):
    mask, order = mask.cpu().numpy(), order.cpu().numpy()
    for b in range(mask.shape[0]):
        vis, msk = order[b, :G - num_mask], order[b, G - num_mask:G]
        assert np.array_equal(vis, np.flatnonzero(mask[b] == 0)) and np.array_equal(msk, np.flatnonzero(mask[b] == 1))
        assert np.all(np.diff(vis) > 0) and np.all(np.diff(msk) > 0)
        assert np.array_equal(np.sort(np.concatenate([vis, msk])), np.arange(G))


@pytest.mark.parametrize("B,G,num_mask,equal", [(3, 64, 38, False), (2, 65, 1, False), (2, 1, 0, False), (2, 512, 307, False),
                                                (2, 100, 99, False), (2, 64, 0, False), (2, 64, 38, True)])
def test_mask_centers_rand_equals_stable_argsort(B, G, num_mask, equal):
    from gm3d_amd._capi import check, lib
    from gm3d_amd.ops import _ptr, _stream
    noise = torch.full((B, G), 0.25) if equal else torch.rand(B, G, generator=torch.Generator().manual_seed(G + num_mask))
    if not equal and G >= 64:
        noise[:, 7] = noise[:, 40]          # a tie: the lower index goes first
        noise[0, 3], noise[0, 5] = 0.0, -0.0
    pitch = G + 3
    mask = torch.full((B, G), 9, dtype=torch.uint8, device="cuda")
    order = torch.full((B, pitch), -7, dtype=torch.int64, device="cuda")
    check(lib.gm3d_mask_centers(_ptr(noise.cuda()), None, 0, B, G, num_mask, _ptr(mask), _ptr(order), pitch, _stream()), "mask_centers")
    want = np.zeros((B, G), dtype=np.uint8)
    idx = np.argsort(noise.numpy(), axis=1, kind="stable")[:, :num_mask]
    np.put_along_axis(want, idx, 1, axis=1)
    assert np.array_equal(mask.cpu().numpy(), want)
    _check_order(mask, order, G, num_mask)
    assert bool((order[:, G:] == -7).all())          # the padding columns are not written


def _block_ref(center, start, num_mask):
    """fp32 restatement: squared distance summed x, y, z, ranked in (value, index) order."""
    c = center.astype(np.float32)
    out = np.zeros(c.shape[:2], dtype=np.uint8)
    for b in range(c.shape[0]):
        d = c[b, start[b]][None, :] - c[b]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32) + d[:, 2] * d[:, 2]
        out[b, np.argsort(d2, kind="stable")[:num_mask]] = 1
    return out


def test_mask_centers_block_equals_the_reference_mask(fx):
    from gm3d_amd import heads
    center = torch.from_numpy(fx["block_cdl2/center"]).cuda()
    start = torch.from_numpy(fx["block_cdl2/start"]).cuda()
    mask, order = heads.mask_centers(center, 38, start=start)
    assert np.array_equal(mask.cpu().numpy(), fx["block_cdl2/mask"])
    _check_order(mask, order, 64, 38)
    assert bool(mask[torch.arange(4), start.long()].all())


@pytest.mark.parametrize("G", [64, 65, 512])
def test_mask_centers_block_equals_fp32_restatement(G):
    from gm3d_amd import heads
    B, num_mask = 3, int(0.6 * G)
    g = torch.Generator().manual_seed(G)
    center = torch.randn(B, G, 3, generator=g)
    center[1, 11] = center[1, 4]                     # two coincident centres: equal keys, the lower index first
    start = torch.tensor([G - 1, 4, 0], dtype=torch.int32)
    mask, order = heads.mask_centers(center.cuda(), num_mask, start=start.cuda())
    assert np.array_equal(mask.cpu().numpy(), _block_ref(center.numpy(), start.numpy(), num_mask))
    _check_order(mask, order, G, num_mask)
    assert bool(mask[1, 4]) and bool(mask[1, 11])


def test_device_draw_masks_exactly_num_mask_uniformly():
    """B = 4096 clouds, noise drawn by the product's own path (MaskTransformer.select with device_mask): exactly 38 masked per
    cloud; per-position frequency within 0.046 of 38 / 64 -- six binomial standard deviations sqrt(0.594 * 0.406 / 4096) = 0.0077."""
    from gm3d_amd.point_mae import MaskTransformer
    torch.manual_seed(123)
    enc = MaskTransformer(PR.config())
    enc.device_mask = True
    center = torch.zeros(4096, 64, 3, device="cuda")
    mask, vis_ids, mask_ids, on_device = enc.select(center)
    assert on_device and mask.dtype == torch.bool and vis_ids.shape == (4096, 26) and mask_ids.shape == (4096, 38)
    assert bool((mask.sum(1) == 38).all())
    freq = mask.float().mean(0).cpu().numpy()
    print("per-position masked frequency: min %.4f max %.4f" % (freq.min(), freq.max()))
    assert np.abs(freq - 38 / 64).max() <= 0.046


# --------------------------------------------------------------------------- L1 patch loss
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,Mn", [(2, 38), (1, 1)])
def test_patch_chamfer_l1_loss_equals_the_op_chain(dtype, B, Mn):
    """heads.PatchChamferL1LossFn against ops.ChamferDistanceL1 on the gathered patches: equal argmins; loss and dpred within the bar
    tests/test_gpu_heads.py holds the L2 patch kernel to (2e-6 of the largest value in fp32, 2^-8 for a bf16 dpred)."""
    from gm3d_amd import heads, ops
    from gm3d_amd import models_mae_learn_loss as M_
    L = 64
    g = torch.Generator().manual_seed(B * 7 + Mn)
    pix = (torch.randn(B, L, 96, generator=g) * 0.3).cuda().to(dtype).requires_grad_(True)
    target = (torch.randn(B, L, 32, 3, generator=g) * 0.3).cuda()
    order = torch.stack([torch.randperm(L, generator=g) for _ in range(B)]).cuda()
    mask_ids = order[:, L - Mn:]
    pred = pix[:, L - Mn:]
    assert heads.patch_chamfer_loss_supported(pred, target, mask_ids)
    mean, matrix = heads.PatchChamferL1LossFn.apply(pred, target, mask_ids)
    got_i1, got_i2 = mean.grad_fn.saved_tensors[3:5]
    (mean * 3.0).backward()
    got_g = pix.grad.clone()
    pix.grad = None
    tg = M_.take(target, mask_ids).reshape(-1, 32, 3)
    p32 = pix[:, L - Mn:].reshape(-1, 32, 3).to(torch.float32)
    want = ops.ChamferDistanceL1()(p32, tg)
    (want * 3.0).backward()
    d1, d2, i1, i2 = ops.chamfer(p32.detach(), tg)
    assert torch.equal(got_i1, i1) and torch.equal(got_i2, i2)
    want_matrix = ((d1.sqrt().mean(1) + d2.sqrt().mean(1)) / 2).reshape(B, Mn)
    print("L1 loss", float(mean), "op chain", float(want))
    assert float((matrix - want_matrix).abs().max()) <= 2e-6 * float(want_matrix.abs().max())
    assert abs(float(mean) - float(want)) <= 2e-6 * abs(float(want))
    scale = float(pix.grad.float().abs().max())
    tol = 2e-6 if dtype == torch.float32 else 2.0 ** -8
    err = float((got_g.float() - pix.grad.float()).abs().max())
    print("dpred err / scale", err / scale)
    assert err <= tol * scale
    assert float(got_g[:, :L - Mn].abs().max()) == 0.0


# --------------------------------------------------------------------------- model against the fixture
def _fixture_step(M, fx, case, monkeypatch, bf16=False, via_noise=False):
    name, mask_type, loss = case
    m = _model(mask_type, loss)
    pts = torch.from_numpy(fx["pts"]).cuda()
    mask = torch.from_numpy(fx[name + "/mask"]).cuda()
    feed = FeedDropPath(fx[name + "/droppath_masks"])
    monkeypatch.setattr(M, "drop_path", feed)
    monkeypatch.setattr(M, "drop_path_scale", feed.scale)
    kw = {"mask": mask}
    if via_noise:       # a noise that ranks exactly the masked groups first
        kw = {"mask_noise": torch.where(mask, 0.0, 1.0)}
    if bf16:
        from gm3d_amd.fused import weight_cache
        weight_cache.pin(m)
        weight_cache.refresh()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(pts.clone(), **kw)
    else:
        out = m(pts.clone(), **kw)
    assert feed.masks == []
    out.backward()
    return m, out.detach()


@pytest.mark.parametrize("case", PR.CASES, ids=[c[0] for c in PR.CASES])
def test_fp32_parity_with_the_reference_fixture(M, fx, case, monkeypatch):
    """The fixture's mask injected (mask=), its DropPath draws replayed: loss and the six recorded gradients within 1e-5 relative
    (gradients: largest error over the tensor's largest entry, and the norm of the whole tensor)."""
    name = case[0]
    m, loss = _fixture_step(M, fx, case, monkeypatch)
    ref = float(fx[name + "/loss"])
    print(name, "loss", float(loss), "fixture", ref, "rel", abs(float(loss) - ref) / abs(ref))
    named = dict(m.named_parameters())
    stride = int(fx["stride"])
    errs = {}
    for k in PR.GRADS:
        errs[k] = rel(PR.picked(named[k].grad, stride), fx[name + "/grad/" + k])
        n = float(fx[name + "/gradnorm/" + k])
        print(name, k, "rel err", errs[k], "norm rel", abs(float(named[k].grad.double().norm()) - n) / n)
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)
    for k in PR.GRADS:
        assert errs[k] <= 1e-5, (k, errs[k])
        n = float(fx[name + "/gradnorm/" + k])
        assert abs(float(named[k].grad.double().norm()) - n) <= 1e-5 * n, k


def test_bf16_loss_against_the_fixture(M, fx, monkeypatch):
    """bf16 (the measured configuration) against the fixture's fp32 loss, under the bar tests/test_gpu_bf16_parity.py applies to its
    Chamfer loss: MULT x the reference's own bf16-autocast error of that loss (pretrain_bf16.npz, the B = 4 gaussian case)."""
    from tests.test_gpu_bf16_parity import MULT
    gold = np.load(os.path.join(GOLD, "pretrain_bf16.npz"))
    bar = MULT * float(gold["b4_gaussian/ac_err::chamfer_mean"])
    for case in PR.CASES:
        _, loss = _fixture_step(M, fx, case, monkeypatch, bf16=True)
        ref = float(fx[case[0] + "/loss"])
        err = abs(float(loss) - ref) / abs(ref)
        print(case[0], "bf16 loss", float(loss), "fp32 fixture", ref, "rel", err, "bar", bar)
        assert err <= bar, case[0]


def test_device_mask_equals_host_ids(M, fx, monkeypatch):
    """The same mask through mask= (ids by argsort) and through gm3d_mask_centers (mask_noise=): equal losses and gradients, bit
    for bit."""
    case = PR.CASES[0]
    ma, la = _fixture_step(M, fx, case, monkeypatch)
    mb, lb = _fixture_step(M, fx, case, monkeypatch, via_noise=True)
    assert torch.equal(la, lb)
    ga, gb = dict(ma.named_parameters()), dict(mb.named_parameters())
    assert all(torch.equal(ga[k].grad, gb[k].grad) for k in ga), [k for k in ga if not torch.equal(ga[k].grad, gb[k].grad)][:5]


def test_defaults_did_not_move():
    """device_mask left at its default: Point_MAE.forward draws the reference's host shuffle from np.random."""
    m = _model(drop_path=0.0)
    seen = []
    select = m.MAE_encoder.select
    m.MAE_encoder.select = lambda *a, **k: seen.append(select(*a, **k)) or seen[-1]
    np.random.seed(11)
    loss = m(clouds.gaussian(4, 1024, seed=5).cuda())
    assert torch.isfinite(loss) and len(seen) == 1 and seen[0][3] is False
    want = m.MAE_encoder._mask_center_rand(torch.zeros(4, 64, 3), rng=np.random.RandomState(11))
    assert torch.equal(seen[0][0].cpu(), want)


# --------------------------------------------------------------------------- the step
def _args(**kw):
    a = dict(bf16=True, lr=1e-3, epochs=300, warmup_epochs=10, step_per_update=1)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("mask_type,B,G,accum", [("rand", 4, 64, 1), ("block", 4, 64, 1), ("rand", 16, 128, 1), ("block", 16, 128, 1),
                                                  ("rand", 4, 64, 2)])
def test_replay_equals_eager(mask_type, B, G, accum):
    """GraphedPointMAEStep with injected draws against pretrain_step fed the same draws, five steps from identical state: loss,
    flat parameters and both moment buffers equal after every step."""
    from gm3d_amd import engine_pretrain_point_mae as EP
    m = _model(mask_type, drop_path=0.0, num_group=G)
    opt = EP.build_optimizer(m)
    args = _args(step_per_update=accum)
    x = [clouds.gaussian(B, 1024, seed=500 + i).cuda() for i in range(5)]
    gen = torch.Generator().manual_seed(17)
    noise = [torch.rand(B, G, generator=gen).cuda() for _ in range(5)]
    start = [torch.randint(0, G, (B,), generator=gen, dtype=torch.int32).cuda() for _ in range(5)]
    g = EP.GraphedPointMAEStep(m, opt, x[0], args, warmup_iters=2 * accum, augment=False, inject_mask_noise=True)
    state = ({k: v.clone() for k, v in m.state_dict().items()}, opt.M.clone(), opt.V.clone(), opt.step_dev.clone())

    def restore():
        with torch.no_grad():
            m.load_state_dict(state[0])
            opt.M.copy_(state[1]); opt.V.copy_(state[2]); opt.step_dev.copy_(state[3])
            opt.sync_shadows()
            if opt.GA is not None:
                opt.GA.zero_()

    restore()
    want = []
    for i in range(5):
        o = EP.pretrain_step(m, opt, x[i].clone(), args, mask_noise=noise[i], mask_start=start[i], augment=False, micro_step=i)
        want.append((o["loss"].clone(), opt.P.clone(), opt.M.clone(), opt.V.clone()))
    restore()
    for i in range(5):
        o = g(x[i], mask_noise=noise[i], mask_start=start[i], update=(i + 1) % accum == 0)
        got = (o["loss"], opt.P, opt.M, opt.V)
        assert bool(torch.isfinite(got[0]))
        assert all(torch.equal(a, b) for a, b in zip(got, want[i])), (i, float(got[0]), float(want[i][0]))
    assert not torch.equal(want[0][1], want[4][1])          # the parameters did move


def test_train_one_epoch(monkeypatch):
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import engine_pretrain_point_mae as EP
    m = _model()
    opt = EP.build_optimizer(m)
    loader = [clouds.gaussian(8, 1024, seed=700 + i) for i in range(8)]          # CPU batches: the engine moves them
    bn = m.MAE_encoder.encoder.first_conv[1]
    before = bn.running_mean.clone()
    replay = EP.GraphedPointMAEStep.__call__

    def no_sync_replay(self, *a, **k):          # a synchronising call inside the replayed part raises
        torch.cuda.set_sync_debug_mode("error")
        try:
            return replay(self, *a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    monkeypatch.setattr(EP.GraphedPointMAEStep, "__call__", no_sync_replay)
    args = _args()
    st = EP.train_one_epoch(m, loader, opt, "cuda", 3, args, print_freq=100)
    assert st["replayed_iters"] == 8 - E.EAGER_WARMUP_ITERS and st["capture_s"] > 0
    assert len(st["step_losses"]) == 8 and all(np.isfinite(st["step_losses"])) and np.isfinite(st["loss"])
    assert abs(st["loss"] - 1000.0 * float(np.mean(st["step_losses"]))) <= 1e-9 * abs(st["loss"])
    assert st["lr"] == EP.cosine_lr(2, 1e-3, 300, 10) and float(opt.lr_dev) == np.float32(st["lr"])
    assert not torch.equal(bn.running_mean, before) and int(bn.num_batches_tracked) == 8
    assert m.MAE_encoder.device_mask
    st2 = EP.train_one_epoch(m, loader, opt, "cuda", 4, args, print_freq=100)          # the captured step outlives the epoch
    assert st2["replayed_iters"] == 8 and st2["capture_s"] == 0.0 and float(opt.lr_dev) == np.float32(EP.cosine_lr(3, 1e-3, 300, 10))


def test_checkpoint_is_the_published_runs_teacher(tmp_path):
    from gm3d_amd import engine_pretrain_Classifier_SVM as EV
    from gm3d_amd import engine_pretrain_point_mae as EP
    from gm3d_amd.point_mae import Point_MAE
    from gm3d_amd.point_transformer import PointTransformer
    from tests.test_gpu_published import TCFG, _args as published_args, build
    m = _model(drop_path=0.0)
    opt = EP.build_optimizer(m)
    m.MAE_encoder.device_mask = True
    for i in range(2):
        EP.pretrain_step(m, opt, clouds.gaussian(4, 1024, seed=800 + i).cuda(), _args())
    path = EP.save_checkpoint(str(tmp_path / "ckpt-last.pth"), m, opt, epoch=0, metrics={"acc": 0.0}, best_metrics={"acc": 0.0})
    teacher = EP.load_teacher(path, Point_MAE(TCFG)).cuda()
    assert all(torch.equal(a, b) for a, b in zip(teacher.state_dict().values(), m.state_dict().values()))
    student, _ = build(21, 22, drop_path=0.0)
    student.train()
    ema = EV.ModelEma(student, decay=0.999)
    popt = EV.build_optimizer(student, lr=1e-3, weight_decay=0.05)
    out = EV.pretrain_step(student, ema, teacher, popt, clouds.gaussian(4, 1024, seed=91).cuda(), 150, published_args(), augment=False)
    assert all(bool(torch.isfinite(out[k])) for k in ("loss", "loss_learn", "loss_mse", "loss_chfr", "grad_norm"))
    cls = PointTransformer(dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64,
                                encoder_dims=384))
    cls.load_model_from_ckpt(path, key="base_model")
    assert torch.equal(cls.blocks.blocks[0].mlp.fc1.weight.cpu(), m.MAE_encoder.blocks.blocks[0].mlp.fc1.weight.cpu())

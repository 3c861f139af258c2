"""-m gpu: the Point-M2AE classifiers (gm3d_amd/point_m2ae_cls.py) and their classification tail (gm3d_amd/csrc/cls_tail.hip).

  * the tail (ops.cls_tail) against an aten restatement written here: both pool modes, B in {2, 40, 128}, injected dropout factors,
    logits, loss, running statistics and every gradient; an exact max-pool tie; eval mode against module.eval();
  * the classifier against the CPU oracle (oracle/hier_ref.m2ae_forward's features + the head restated here), fp32, gradients
    judged against an fp64 run of the same computation with the product's discrete decisions injected (tests/test_gpu_m2ae.py);
  * a saved PointM2AE checkpoint loads and reproduces PointM2AE(pts, noaug=True) bit for bit;
  * GraphedFinetuneStep with the classifier against eager finetune_step; a short bf16 training run learns."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import clouds

pytestmark = pytest.mark.gpu

MODELNET = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
                encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=40)
SCAN = dict(MODELNET, NAME="Point_M2AE_ScanObjectNN", group_sizes=[32, 16, 16], cls_dim=15)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _head(F_in, cls_dim, seed):
    torch.manual_seed(seed)
    h = nn.Sequential(nn.Linear(F_in, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
                      nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5), nn.Linear(256, cls_dim))
    with torch.no_grad():
        for bn in (h[1], h[5]):
            bn.weight.uniform_(0.8, 1.2)
            bn.bias.uniform_(-0.1, 0.1)
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    return h


def _pool_first(x, mode):
    """mean and max over tokens, the max taken at the LOWEST index among tied maxima (so its gradient lands there)."""
    T = x.shape[1]
    mx = x.detach().max(dim=1, keepdim=True)[0]
    ar = torch.arange(T, device=x.device).view(1, T, 1)
    idx = torch.where(x.detach() == mx, ar, T).min(dim=1, keepdim=True)[0]
    m = x.gather(1, idx).squeeze(1)
    mean = x.mean(1)
    return mean + m if mode == 0 else torch.cat([mean, m], dim=-1)


def aten_tail(x, head, mode, training, drop=None, labels=None):
    """The restatement: pool, Linear, BatchNorm (training: batch statistics + running update; eval: running), ReLU, x dropout
    factor, Linear, BatchNorm, ReLU, x factor, Linear; mean cross-entropy."""
    l1, bn1, l2, bn2, l3 = head[0], head[1], head[4], head[5], head[8]
    f = _pool_first(x.float() if x.dtype != torch.float64 else x, mode)

    def bn(y, m):
        return F.batch_norm(y, m.running_mean, m.running_var, m.weight, m.bias, training, m.momentum, m.eps)
    if training:
        for m in (bn1, bn2):
            m.num_batches_tracked += 1
    a = torch.relu(bn(l1(f), bn1))
    if training and drop is not None:
        a = a * drop[0]
    a = torch.relu(bn(l2(a), bn2))
    if training and drop is not None:
        a = a * drop[1]
    z = l3(a)
    return z if labels is None else (z, F.cross_entropy(z, labels))


def _head_params(h):
    return [h[0].weight, h[0].bias, h[1].weight, h[1].bias, h[4].weight, h[4].bias, h[5].weight, h[5].bias, h[8].weight, h[8].bias]


def _tail_case(B, mode, dtype, training=True, drop_p=0.5, T=64, cls_dim=40, seed=0):
    from gm3d_amd import ops
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(B, T, 384, generator=g).cuda().to(dtype)
    labels = torch.randint(0, cls_dim, (B,), generator=g).cuda()
    w = torch.randn(B, cls_dim, generator=g).cuda()
    drop = ((torch.rand(2, B, 256, generator=g) >= drop_p).float() / (1 - drop_p)).cuda() if drop_p else None
    hk = _head(384 * (2 if mode else 1), cls_dim, seed + 1).cuda().train(training)
    ha = copy.deepcopy(hk)
    xk = x0.clone().requires_grad_(True)
    xa = x0.clone().requires_grad_(True)
    zk, lk = ops.cls_tail(xk, hk, mode, training, drop=drop, labels=labels)
    za, la = aten_tail(xa, ha, mode, training, drop=drop, labels=labels)
    if training:
        (lk + (zk * w).sum()).backward()
        (la + (za * w).sum()).backward()
    if dtype != torch.float32:
        return (xk, hk, zk, lk), (xa, ha, za, la)
    # the same computation in fp64 (same dropout factors, same labels): the truth both fp32 results are judged against
    hd = _head(384 * (2 if mode else 1), cls_dim, seed + 1).cuda().double().train(training)
    xd = x0.double().clone().requires_grad_(True)
    zd, ld = aten_tail(xd, hd, mode, training, drop=None if drop is None else drop.double(), labels=labels)
    if training:
        (ld + (zd * w.double()).sum()).backward()
    return (xk, hk, zk, lk), (xa, ha, za, la), (xd, hd, zd, ld)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B", [2, 40, 128])
def test_tail_fp32_against_aten(B, mode):
    """Every result within 1e-5 of the fp64 restatement, or within 3x the fp32 restatement's own distance from it where fp32 cannot
    do better (at B = 2 a training-mode BatchNorm is nearly constant in its input: the input-side gradients are cancellation
    residue of the same size in any fp32 evaluation)."""
    (xk, hk, zk, lk), (xa, ha, za, la), (xd, hd, zd, ld) = _tail_case(B, mode, torch.float32)

    def ok(k, a, d, what):
        ek, ea = _rel(k, d), _rel(a, d)
        assert ek <= max(1e-5, 3.0 * ea), (what, ek, ea)
    ok(zk, za, zd, "logits")
    ok(lk, la, ld, "loss")
    for i, (bk, ba, bd) in enumerate(((hk[1], ha[1], hd[1]), (hk[5], ha[5], hd[5]))):
        ok(bk.running_mean, ba.running_mean, bd.running_mean, "running_mean%d" % i)
        ok(bk.running_var, ba.running_var, bd.running_var, "running_var%d" % i)
        assert int(bk.num_batches_tracked) == int(ba.num_batches_tracked) == 1
    ok(xk.grad, xa.grad, xd.grad, "dx")
    gscale = float(_head_params(hd)[0].grad.abs().max())
    for i, (pk, pa, pd) in enumerate(zip(_head_params(hk), _head_params(ha), _head_params(hd))):
        if i in (1, 5):      # biases in front of a training-mode BatchNorm: the true gradient is 0, both report rounding residue
            assert float(pk.grad.abs().max()) <= 1e-5 * gscale + 1e-6, i
            continue
        ok(pk.grad, pa.grad, pd.grad, "param%d" % i)


@pytest.mark.parametrize("mode", [0, 1])
def test_tail_bf16_input_within_band(mode):
    (xk, hk, zk, lk), (xa, ha, za, la) = _tail_case(40, mode, torch.bfloat16)
    assert xk.grad.dtype == torch.bfloat16
    assert _rel(zk, za) <= 5e-2 and _rel(lk, la) <= 5e-2
    assert _rel(xk.grad.float(), xa.grad.float()) <= 5e-2
    for i, (pk, pa) in enumerate(zip(_head_params(hk), _head_params(ha))):
        if i not in (1, 5):
            assert _rel(pk.grad, pa.grad) <= 5e-2, i


def test_tail_max_pool_tie_goes_to_the_lowest_index():
    from gm3d_amd import ops
    B, T = 4, 16
    x = torch.randn(B, T, 384).cuda()
    top = x.max(dim=1)[0] + 1.0   # an exact tie between tokens 3 and 9 in every channel, above every other token
    x[:, 3, :] = top
    x[:, 9, :] = top
    x.requires_grad_(True)
    head = _head(384, 40, 3).cuda()
    z = ops.cls_tail(x, head, 0, True)
    z.sum().backward()
    g = x.grad
    mean_part = g[:, 0, :]                                        # token 0 receives only the mean's share
    assert torch.equal(g[:, 9, :], mean_part) and torch.equal(g[:, 5, :], mean_part)
    assert not torch.equal(g[:, 3, :], mean_part)


@pytest.mark.parametrize("mode", [0, 1])
def test_tail_eval_mode_against_module_eval(mode):
    from gm3d_amd import ops
    torch.manual_seed(4)
    x = torch.randn(40, 64, 384).cuda()
    head = _head(384 * (2 if mode else 1), 15, 5).cuda().eval()
    before = [t.clone() for t in (head[1].running_mean, head[1].running_var, head[1].num_batches_tracked)]
    with torch.no_grad():
        zk = ops.cls_tail(x, head, mode, False)
        f = x.mean(1) + x.max(1)[0] if mode == 0 else torch.cat([x.mean(1), x.max(1)[0]], -1)
        za = head(f)
    assert _rel(zk, za) <= 1e-5
    assert all(torch.equal(a, b) for a, b in zip(before, (head[1].running_mean, head[1].running_var, head[1].num_batches_tracked)))


# --------------------------------------------------------------------------- the classifier against the oracle
def _classifier(cfg, seed=3):
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_m2ae import PointM2AE
    from oracle import model_ref as R
    pre = PointM2AE({k: v for k, v in cfg.items() if k in ("group_sizes", "num_groups", "encoder_depths", "encoder_dims",
                                                            "local_radius", "num_heads")})
    R.det_fill_(pre, seed=seed)
    torch.manual_seed(seed)
    m = C.build_model(cfg)
    m.load_pretrained_state(pre.state_dict())
    for mod in m.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    return pre, m


def _head_ref(hd, x, mode, win=None, signs=None):
    """the head restated over a dict of tensors; win (B,T,C) injects the max-pool winners, signs the two ReLU sign patterns."""
    mean = x.mean(1)
    mx = (x * win).sum(1) if win is not None else x.max(1)[0]
    f = mean + mx if mode == 0 else torch.cat([mean, mx], -1)
    outs = []
    for i, (l, b) in enumerate((("0", "1"), ("4", "5"))):
        y = f @ hd[l + ".weight"].t() + hd[l + ".bias"]
        y = F.batch_norm(y, None, None, hd[b + ".weight"], hd[b + ".bias"], True, 0.1, 1e-5)
        outs.append(y.detach() > 0)
        f = torch.where(signs[i], y, torch.zeros((), dtype=y.dtype)) if signs is not None else torch.relu(y)
    return f @ hd["8.weight"].t() + hd["8.bias"], outs


@pytest.mark.parametrize("cfg,npts", [(MODELNET, 1024), (SCAN, 2048)], ids=["modelnet40", "scanobjectnn"])
def test_classifier_against_oracle(cfg, npts, monkeypatch):
    from gm3d_amd import point_m2ae as P
    from oracle import hier_ref as HR
    from oracle import ops as oracle_ops
    oracle_ops.build()
    B = 4          # (at B = 2 the head's training-mode BatchNorms are nearly constant: every upstream gradient is cancellation residue)
    mode = 0 if cfg is MODELNET else 1
    pre, m = _classifier(cfg)
    pts = clouds.gaussian(B, npts, seed=11)
    labels = torch.tensor([1, cfg["cls_dim"] - 1, 3, 0])
    m = m.cuda().train()
    P.POOL_TAPS, P.ACT_TAPS = [], []
    try:
        logits = m(pts.cuda())
        pool_idx, act_signs = [t.cpu() for t in P.POOL_TAPS], [t.cpu() for t in P.ACT_TAPS]
    finally:
        P.POOL_TAPS = P.ACT_TAPS = None
    assert len(pool_idx) == 6 and len(act_signs) == 6
    loss = F.cross_entropy(logits, labels.cuda())
    loss.backward()
    # the head's decisions, from the product's own tokens
    with torch.no_grad():
        xp = m.forward_tokens(pts.cuda()).cpu()
    mx = xp.max(1, keepdim=True)[0]
    first = torch.where(xp == mx, torch.arange(xp.shape[1]).view(1, -1, 1), xp.shape[1]).min(1, keepdim=True)[0]
    win = torch.zeros_like(xp).scatter_(1, first, 1.0)
    hsd = {k[len("cls_head_finetune."):]: v.detach().cpu() for k, v in m.state_dict().items() if k.startswith("cls_head_finetune.")}
    _, head_signs = _head_ref(hsd, xp, mode)
    # the decoder part of m2ae_forward runs too (its features are taken before it): sign patterns of the right sizes for it
    gcfg = dict(HR.CFG, group_sizes=tuple(cfg["group_sizes"]))
    pad = [torch.ones(B * 64 * 1024, dtype=torch.bool), torch.ones(B * 256 * 768, dtype=torch.bool), torch.ones(B * 256 * 192, dtype=torch.bool)]
    base = pre.state_dict()
    # the classifier masks nothing at any level; the oracle's pretraining forward back-projects the coarse visibility (a finer token no
    # coarse group contains counts as masked): here every level is visible
    monkeypatch.setattr(HR, "propagate_visibility", lambda mask_coarse, idxs: [torch.zeros(B, i.shape[1], dtype=torch.bool) for i in idxs])

    def run(dt):
        sd = {k: (v.detach().to(dt).clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in base.items()}
        hd = {k: (v.detach().to(dt).clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in hsd.items()}
        del HR.DECISION_MARGINS[:]
        feats = HR.m2ae_forward(sd, pts, None, training=True, cfg=gcfg, pool_idx=pool_idx, act_signs=act_signs + pad)["features"]
        z, _ = _head_ref(hd, feats, mode, win=win.to(dt), signs=head_signs)
        lo = F.cross_entropy(z, labels)
        lo.backward()
        return sd, hd, z, lo

    sd32, hd32, z32, l32 = run(torch.float32)
    # the injected decisions are the oracle's own up to rounding (the last three entries: the padded decoder signs)
    worst = max((mg for kind, mg in HR.DECISION_MARGINS[:-3] if kind in ("sign", "pool")), default=0.0)
    assert worst <= 1e-4, worst
    sd64, hd64, z64, l64 = run(torch.float64)
    for what, prod, c32, c64 in (("logits", logits, z32, z64), ("loss", loss, l32, l64)):
        # within 1e-5 of the fp32 oracle, or as close to the fp64 run as the fp32 oracle is (x3)
        assert _rel(prod, c32) <= 1e-5 or _rel(prod, c64) <= 3.0 * _rel(c32, c64), (what, _rel(prod, c32), _rel(prod, c64), _rel(c32, c64))
    grads64 = {}
    for name, _ in m.named_parameters():
        if name.startswith("cls_head_finetune."):
            k = name[len("cls_head_finetune."):]
            grads64[name] = (hd64[k].grad, hd32[k].grad)
        else:
            k = "encoder_norms.2." + name[len("norm."):] if name.startswith("norm.") else name
            grads64[name] = (sd64[k].grad, sd32[k].grad)
    gscale = max(float(g64.abs().max()) for g64, _ in grads64.values() if g64 is not None)
    bad, rows = {}, 0
    for name, p in m.named_parameters():
        g64, g32 = grads64[name]
        if p.grad is None:
            assert g64 is None or float(g64.abs().max()) <= 1e-9 * gscale, name
            continue
        rows += 1
        scale = max(float(g64.abs().max()), 1e-4 * gscale)
        e_prod = float((p.grad.detach().cpu().double() - g64.double()).abs().max()) / scale
        e_cpu = float((g32.double() - g64.double()).abs().max()) / scale
        zero = float(g64.abs().max()) <= 1e-9 * gscale
        # floor 5e-4, not test_gpu_m2ae's 5e-5: every gradient passes through the head's two training-mode BatchNorms over B = 4
        # rows, which amplify the last-bit differences of the encoder's features (the fp32 CPU restatement itself is 6e-5 from fp64)
        if e_prod > (max(3e-3, 3.0 * e_cpu) if zero else max(5e-4, 3.0 * e_cpu)):
            bad[name] = (e_prod, e_cpu)
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1][0])[:8]
    assert rows > 150


@pytest.mark.parametrize("bf16", [False, True])
def test_checkpoint_tokens_equal_the_pretrained_encoder_bit_for_bit(tmp_path, bf16):
    """The classifier's tokens = the pretrained model's coarsest encoder output with nothing masked at any level, after
    encoder_norms.2.  (PointM2AE(pts, noaug=True) back-projects an all-visible coarse mask, which still hides the finer tokens that
    no coarser group contains: equal to this exactly when every finer token is covered.)"""
    from gm3d_amd import checkpoint
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_m2ae import PointM2AE
    from oracle import model_ref as R
    pre = R.det_fill_(PointM2AE(), seed=6)
    path = str(tmp_path / "pre.pth")
    checkpoint.save_checkpoint(path, pre, epoch=0, model_name="Point_M2AE")
    m = C.build_model(MODELNET)
    res = m.load_model_from_ckpt(path)
    assert all(k.startswith("cls_head_finetune.") for k in res.missing_keys)
    pre, m = pre.cuda().eval(), m.cuda().eval()
    pts = clouds.uniform(3, 2048, seed=8).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
        group = pre.group_divider(pts)
        want = pre.encoder_norms[2](pre.encode(*group, None)[2])
        got = m.forward_tokens(pts, group=group)
        if not bf16:
            masks = pre(pts, group=group)["masks"]
            if not any(bool(mk.any()) for mk in masks):
                assert torch.equal(got, pre(pts, group=group, noaug=True))
    assert got.dtype == want.dtype and torch.equal(got, want)


# --------------------------------------------------------------------------- the engine
def _run_steps(graphed, bf16, batches, targets):
    from gm3d_amd import engine_finetune as EF
    crit = nn.CrossEntropyLoss()
    args = SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=0, epochs=300)
    _, m = _classifier(MODELNET, seed=9)
    m = m.cuda().train()
    opt = EF.build_optimizer(m, lr=1e-3, capturable=True, flat=True, max_norm=10.0)
    EF.adjust_learning_rate(opt, 5.0, args)
    rng = np.random.RandomState(7)
    if graphed:
        g = EF.GraphedFinetuneStep(m, crit, opt, batches[0], targets, npoints=1024, max_norm=10.0, bf16=bf16, rng=rng, augment=False,
                                   warmup_iters=3)
        step = lambda x: g(x, targets)
    else:
        sub = rng.choice(1200, 1024, False)
        for _ in range(3):
            EF.finetune_step(m, crit, opt, batches[0], targets, npoints=1024, max_norm=10.0, bf16=bf16, subset=sub, augment=False)
        step = lambda x: EF.finetune_step(m, crit, opt, x, targets, npoints=1024, max_norm=10.0, bf16=bf16,
                                          subset=rng.choice(1200, 1024, False), augment=False)
    guards = [torch.full((n,), 12345.0, device="cuda") for n in (1, 2, 8, 64, 1024, 1 << 18) for _ in range(64)] if graphed else []
    ints = [torch.full((), 777, dtype=torch.int64, device="cuda") for _ in range(128)] if graphed else []
    poison = [torch.full((n,), float("nan"), device="cuda") for n in (1, 4, 16, 96, 384, 1536, 1 << 14, 1 << 20) for _ in range(64)] if graphed else []
    losses, logits = [], []
    for x in batches:
        out = step(x)
        losses.append(out["loss"].clone())
        logits.append(out["outputs"].clone())
    torch.cuda.synchronize()
    assert all(bool((t == 12345.0).all()) for t in guards) and all(int(t) == 777 for t in ints)
    del poison
    return losses, logits, {k: v.detach().clone() for k, v in m.named_parameters()}


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_graph_replay_equals_eager(bf16):
    batches = [clouds.gaussian(8, 2048, seed=50 + i).cuda() for i in range(3)]
    targets = (torch.arange(8).cuda() * 3) % 40
    le, ze, pe = _run_steps(False, bf16, batches, targets)
    lg, zg, pg = _run_steps(True, bf16, batches, targets)
    if bf16:
        assert all(torch.equal(a, b) for a, b in zip(le, lg))
        assert all(torch.equal(a, b) for a, b in zip(ze, zg))
        assert all(torch.equal(pg[k], pe[k]) for k in pe)
    else:
        le_, lg_ = [float(v) for v in le], [float(v) for v in lg]
        assert max(abs(a - b) for a, b in zip(le_, lg_)) <= 1e-5 * max(le_)
        assert max(_rel(pg[k], pe[k]) for k in pe) <= 1e-5


def test_bf16_training_learns_and_evaluates():
    from gm3d_amd import engine_finetune as EF
    _, m = _classifier(dict(MODELNET, cls_dim=2), seed=12)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.5
    m = m.cuda().train()
    crit = nn.CrossEntropyLoss()
    opt = EF.build_optimizer(m, lr=5e-4, weight_decay=0.05)
    B = 16
    pts = torch.cat([clouds.uniform(B // 2, 2048, seed=1), clouds.gaussian(B // 2, 2048, seed=2)]).cuda()
    y = torch.tensor([0] * (B // 2) + [1] * (B // 2)).cuda()
    rng = np.random.RandomState(0)
    losses = []
    for it in range(20):
        out = EF.finetune_step(m, crit, opt, pts, y, npoints=1024, max_norm=10.0, bf16=True,
                               subset=rng.choice(1200, 1024, False))
        losses.append(float(out["loss"]))
    assert all(np.isfinite(losses))
    assert np.mean(losses[-4:]) < np.mean(losses[:4]), losses
    loader = [(None, None, (pts[:8], y[:8])), (None, None, (pts[8:], y[8:]))]
    res = EF.evaluate(loader, m, "cuda", npoints=1024, bf16=True)
    assert res["n"] == B and np.isfinite(res["acc1"]) and np.isfinite(res["loss"])

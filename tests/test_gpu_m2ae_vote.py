"""-m gpu: voting evaluation of the Point-M2AE classifiers (engine_finetune.validate_vote / GraphedVoteEval with
gm3d_amd/point_m2ae_cls.py) on gm3d_vote_sample and gm3d_cls_tail_vote_pool.

Bars, as in tests/test_gpu_vote.py: f32 logits within 1e-5 relative (of the largest magnitude) of the reference loop and of the fp64
restatement; predictions equal where the top-2 margin decides; bf16 input within the 5e-2 band of test_gpu_m2ae_cls against the
autocast aten head.  The pooled feature is bit-equal to the one gm3d_cls_tail_fwd feeds its head."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import model_ref as R
from tests import clouds
from tests.test_gpu_model import rel
from tests.test_gpu_vote import BF16_BAR, device_draws, reference_votes
from tests.test_gpu_vote import build as build_mae

pytestmark = pytest.mark.gpu

MODELNET = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
                encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=40)
SCAN = dict(MODELNET, NAME="Point_M2AE_ScanObjectNN", group_sizes=[32, 16, 16], cls_dim=15)
CASES = [(MODELNET, 1024), (SCAN, 2048)]
IDS = ["modelnet40", "scanobjectnn"]


def build(cfg, seed=3):
    """A classifier with deterministic weights, no DropPath / Dropout, and non-trivial BatchNorm running statistics."""
    from gm3d_amd import point_m2ae_cls as C
    torch.manual_seed(seed)
    m = C.build_model(cfg)
    R.det_fill_(m, seed=seed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in (m.cls_head_finetune[1], m.cls_head_finetune[5]):
            bn.running_mean.copy_(torch.rand(256, generator=g) * 0.4 - 0.2)
            bn.running_var.copy_(torch.rand(256, generator=g) + 0.5)
    for mod in m.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    return m.cuda()


def _margin(mean):
    top = mean.double().topk(2, dim=-1)[0]
    return (top[:, 0] - top[:, 1]).cpu()


# --------------------------------------------------------------------------- 1. the reference's loop
@pytest.mark.parametrize("cfg,npoints", CASES, ids=IDS)
def test_validate_vote_equals_the_reference_loop(cfg, npoints):
    """fp32, B = 4, V = 10, seeded np.random: per vote gather + transform + model(points) in eval mode, then the vote mean and
    torch.max -- per-vote logits and means within 1e-5, predictions equal wherever the top-2 margin exceeds 1e-4."""
    from gm3d_amd import engine_finetune as EF
    m = build(cfg).train()
    V, B = 10, 4
    loader = [(None, None, (clouds.gaussian(B, 2048, seed=60 + i), torch.tensor([1, 2, 3, 4]) * (i + 1) % cfg["cls_dim"]))
              for i in range(2)]
    np.random.seed(21)
    res = EF.validate_vote(m, loader, "cuda", npoints=npoints, times=V, bf16=False, outputs=True)
    assert m.training
    np.random.seed(21)
    m.eval()
    want_votes, want_preds, labels = [], [], []
    with torch.no_grad():
        for _, _, (pts, lab) in loader:
            pts = pts.cuda()
            point_all = EF.vote_point_all(npoints, pts.size(1))
            subsets, scale, shift = device_draws(np.random, point_all, npoints, V, B)
            votes = reference_votes(m, pts, subsets, scale, shift, point_all)
            want_votes.append(votes)
            want_preds.append(torch.max(torch.cat([v.unsqueeze(0) for v in votes]).mean(0), -1)[1])
            labels.append(lab)
    wv = torch.cat(want_votes, dim=1)
    wm = wv.mean(0)
    assert res["n"] == 2 * B
    assert rel(res["votes"], wv) <= 1e-5
    assert rel(res["mean"], wm) <= 1e-5
    decided = _margin(wm) > 1e-4 * float(wm.abs().max())
    assert decided.sum() >= 6
    wp = torch.cat(want_preds).cpu()
    assert torch.equal(res["pred"].cpu()[decided], wp[decided])
    lab = torch.cat(labels)
    assert res["acc_vote"] == float(torch.tensor(int((res["pred"].cpu() == lab).sum())) / float(2 * B) * 100.)


# --------------------------------------------------------------------------- 2. the kernel against fp64 / aten restatements
def _head(F_in, cls_dim, seed):
    h = nn.Sequential(nn.Linear(F_in, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
                      nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5), nn.Linear(256, cls_dim))
    return R.det_fill_(h, seed=seed).cuda().eval()


def _pool(x, mode):
    mean, mx = x.mean(1), x.max(1)[0]
    return mean + mx if mode == 0 else torch.cat([mean, mx], dim=-1)


def _head64(head, f):
    """the eval head in fp64 on the fp64 feature f"""
    p = {k: v.detach().double() for k, v in head.state_dict().items()}
    a = f
    for l, b in (("0", "1"), ("4", "5")):
        a = a @ p[l + ".weight"].t() + p[l + ".bias"]
        a = torch.relu(F.batch_norm(a, p[b + ".running_mean"], p[b + ".running_var"], p[b + ".weight"], p[b + ".bias"], False, 0.0,
                                    head[int(b)].eps))
    return a @ p["8.weight"].t() + p["8.bias"]


def _fwd_feat(x, head, mode):
    """gm3d_cls_tail_fwd's eval-mode pooled feature, in chunks of at most 128 rows (its batch limit)."""
    from gm3d_amd import ops
    from gm3d_amd._capi import lib
    l1, bn1, l2, bn2, l3 = ops._tail_head(head)
    R_, T, C = x.shape
    Fw, cls_dim = l1.weight.size(1), l3.weight.size(0)
    out = []
    for i in range(0, R_, 128):
        xc = x[i:i + 128]
        B = xc.size(0)
        feat = torch.empty(B, Fw, device="cuda")
        argmax = torch.empty(B, C, dtype=torch.int32, device="cuda")
        h = torch.empty(2, B, 256, device="cuda")
        stats = torch.empty(4, 256, device="cuda")
        logits = torch.empty(B, cls_dim, device="cuda")
        ops._launch("gm3d_cls_tail_fwd", {}, lib.gm3d_cls_tail_fwd, ops._ptr(xc), B, T, C, mode,
                    *[ops._ptr(p) for p in (l1.weight, l1.bias, bn1.weight, bn1.bias, l2.weight, l2.bias, bn2.weight, bn2.bias,
                                            l3.weight, l3.bias)], cls_dim,
                    ops._ptr(bn1.running_mean), ops._ptr(bn1.running_var), ops._ptr(bn1.num_batches_tracked),
                    ops._ptr(bn2.running_mean), ops._ptr(bn2.running_var), ops._ptr(bn2.num_batches_tracked), float(bn1.eps),
                    float(bn1.momentum), 0, None, None, ops._ptr(feat), ops._ptr(argmax), ops._ptr(h), ops._ptr(stats),
                    ops._ptr(logits), None, ops._DT[x.dtype], ops._stream())
        out.append(feat)
    return torch.cat(out)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


KERNEL_CASES = [(1, 1, 64, 15), (10, 40, 64, 40), (16, 41, 512, 256), (10, 41, 512, 15), (16, 40, 64, 256), (1, 40, 512, 40),
                (10, 1, 512, 256)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("V,B,T,cls_dim", KERNEL_CASES, ids=["V%d-B%d-T%d-c%d" % c for c in KERNEL_CASES])
def test_cls_tail_vote_pool_against_restatements(V, B, T, cls_dim, mode):
    from gm3d_amd import ops
    head = _head(768 if mode else 384, cls_dim, seed=V * 1000 + T + cls_dim + mode)
    g = torch.Generator(device="cuda").manual_seed(V * B * T + cls_dim + mode)
    x = torch.randn(V * B, T, 384, device="cuda", generator=g)
    for dt in (torch.float32, torch.bfloat16):
        xx = x.to(dt)
        f64 = _pool(xx.double(), mode)
        want64 = _head64(head, f64).view(V, B, cls_dim)
        with torch.no_grad():
            aten = head(_pool(xx.float(), mode)).view(V, B, cls_dim)
        labels = want64.mean(0).argmax(-1)
        labels[::2] = (labels[::2] + 1) % cls_dim
        correct = torch.full((1,), 3, dtype=torch.long, device="cuda")
        votes = torch.empty(V, B, cls_dim, device="cuda")
        feat = torch.empty(V * B, 768 if mode else 384, device="cuda")
        mean, pred = ops.cls_tail_vote_pool(xx, head, mode, labels, V, correct, votes=votes, feat=feat)
        assert rel(votes, want64) <= 1e-5, dt          # the f32 head on the same (f32 / bf16-valued) tokens
        assert rel(votes, aten) <= 1e-5, dt
        assert rel(mean, want64.mean(0)) <= 1e-5, dt
        assert torch.equal(mean, votes.sum(0) / V) or rel(mean, votes.double().sum(0) / V) <= 1e-6
        assert torch.equal(pred, mean.argmax(-1))
        assert int(correct) == 3 + int((pred == labels).sum())
        assert _bits_equal(feat, _fwd_feat(xx, head, mode)), dt
        if dt == torch.bfloat16:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                ac = head(_pool(xx, mode)).float().view(V, B, cls_dim)
            assert rel(votes, ac) <= BF16_BAR
    # the running statistics are read on every call
    head[1].running_var.mul_(2.0)
    mean2, _ = ops.cls_tail_vote_pool(x, head, mode, labels, V, correct)
    assert rel(mean2, _head64(head, _pool(x.double(), mode)).view(V, B, cls_dim).mean(0)) <= 1e-5


def test_argmax_tie_goes_to_the_lowest_index():
    from gm3d_amd import ops
    V, B, cls_dim = 10, 5, 40
    head = _head(384, cls_dim, seed=1)
    with torch.no_grad():
        head[8].weight[9] = head[8].weight[4]
        head[8].bias[4] = head[8].bias[9] = 50.0           # classes 4 and 9: identical logits, above every other class
    x = torch.randn(V * B, 64, 384, device="cuda")
    mean, pred = ops.cls_tail_vote_pool(x, head, 0, torch.zeros(B, dtype=torch.long, device="cuda"), V,
                                        torch.zeros(1, dtype=torch.long, device="cuda"))
    assert torch.equal(mean[:, 4], mean[:, 9])
    assert pred.tolist() == [4] * B


def test_nan_wins_in_the_pool_and_the_argmax():
    from gm3d_amd import ops
    V, B, cls_dim = 4, 3, 15
    head = _head(768, cls_dim, seed=2)
    with torch.no_grad():
        head[8].weight[11, 0] = float("nan")               # class 11's logit is NaN in every vote
        head[8].bias[3] = 1000.0                           # class 3 is far above every other number
    x = torch.randn(V * B, 64, 384, device="cuda")
    x[1, 7, 5] = float("nan")                             # vote 0 of cloud 1: channel 5 pools to NaN (mean and max)
    feat = torch.empty(V * B, 768, device="cuda")
    correct = torch.zeros(1, dtype=torch.long, device="cuda")
    mean, pred = ops.cls_tail_vote_pool(x, head, 1, torch.full((B,), 11, dtype=torch.long, device="cuda"), V, correct, feat=feat)
    assert torch.isnan(feat[1, 5]) and torch.isnan(feat[1, 384 + 5])
    assert int(torch.isnan(feat).sum()) == 2
    assert _bits_equal(feat, _fwd_feat(x, head, 1))
    assert bool(torch.isnan(mean[:, 11]).all()) and bool((mean[:, 3] > 500).all())
    assert pred.tolist() == [11] * B                       # a NaN logit wins over every number (torch.max)
    assert int(correct) == B


# --------------------------------------------------------------------------- 3.-5. the engine
def _loader(sizes, cls_dim, seed):
    return [(None, None, (clouds.gaussian(n, 2048, seed=seed + i), (torch.arange(n) * 7 + i) % cls_dim)) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("cfg,npoints", CASES, ids=IDS)
def test_graph_equals_eager_bf16(cfg, npoints):
    """B = 40, V = 10, bf16: the graph replays equal the eager pass bit for bit; the ragged last batch of 17 runs eagerly with the
    same draws in both."""
    from gm3d_amd import engine_finetune as EF
    m = build(cfg, seed=8)
    loader = _loader([40, 40, 17], cfg["cls_dim"], 300)
    g = EF.validate_vote(m, loader, "cuda", npoints=npoints, bf16=True, rng=np.random.RandomState(11), graphed=True, outputs=True)
    e = EF.validate_vote(m, loader, "cuda", npoints=npoints, bf16=True, rng=np.random.RandomState(11), graphed=False, outputs=True)
    for k in ("votes", "mean", "pred"):
        assert torch.equal(g[k], e[k]), k
    assert g["acc_vote"] == e["acc_vote"] and g["n"] == e["n"] == 97
    assert g["votes"].shape == (10, 97, cfg["cls_dim"])


@pytest.mark.parametrize("cfg", [MODELNET, SCAN], ids=IDS)
def test_graph_outlives_training(cfg):
    from gm3d_amd import engine_finetune as EF
    m = build(cfg, seed=9)
    pts = clouds.gaussian(4, 2048, seed=400)
    labels = torch.tensor([1, 5, 9, 13]) % cfg["cls_dim"]
    loader = [(None, None, (pts, labels))]
    opt = EF.build_optimizer(m, lr=1e-3, flat=True, max_norm=10.0)
    ge = EF.GraphedVoteEval(m, pts.cuda(), labels.cuda(), bf16=True, rng=np.random.RandomState(3), keep_votes=True)
    graph = ge.graph
    before = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=ge, outputs=True)
    m.train()
    step = EF.GraphedFinetuneStep(m, nn.CrossEntropyLoss(), opt, clouds.gaussian(8, 2048, seed=401).cuda(),
                                  (torch.arange(8) * 5 % cfg["cls_dim"]).cuda(), npoints=1024, bf16=True,
                                  rng=np.random.RandomState(2), augment=False, warmup_iters=3)
    for i in range(3):
        step(clouds.gaussian(8, 2048, seed=410 + i).cuda(), (torch.arange(8) * 3 % cfg["cls_dim"]).cuda())
    torch.cuda.synchronize()
    after = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=ge, outputs=True)
    assert ge.graph is graph                               # replayed, not captured again
    assert m.training
    eager = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=False, outputs=True)
    assert not torch.equal(before["votes"], after["votes"])
    for k in ("votes", "mean", "pred"):
        assert torch.equal(after[k], eager[k]), k


@pytest.mark.parametrize("cfg,npoints", CASES, ids=IDS)
def test_bf16_preds_match_fp32_where_decided(cfg, npoints):
    from gm3d_amd import engine_finetune as EF
    m = build(cfg, seed=12)
    loader = _loader([16, 16], cfg["cls_dim"], 500)
    f32 = EF.validate_vote(m, loader, "cuda", npoints=npoints, bf16=False, rng=np.random.RandomState(4), outputs=True)
    b16 = EF.validate_vote(m, loader, "cuda", npoints=npoints, bf16=True, rng=np.random.RandomState(4), outputs=True)
    decided = _margin(f32["mean"]) > 2 * BF16_BAR * float(f32["mean"].abs().max())
    assert decided.sum() >= 1
    assert torch.equal(b16["pred"].cpu()[decided], f32["pred"].cpu()[decided])


# --------------------------------------------------------------------------- 6. Point-MAE keeps its tail
def test_point_mae_vote_still_calls_cls_tail_vote(monkeypatch):
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    calls = []
    orig = ops.cls_tail_vote

    def spy(*a, **k):
        calls.append("cls_tail_vote")
        return orig(*a, **k)

    monkeypatch.setattr(ops, "cls_tail_vote", spy)
    monkeypatch.setattr(ops, "cls_tail_vote_pool", lambda *a, **k: calls.append("cls_tail_vote_pool"))
    m = build_mae(seed=5)
    loader = [(None, None, (clouds.gaussian(4, 2048, seed=700), torch.tensor([1, 2, 3, 4])))]
    res = EF.validate_vote(m, loader, "cuda", bf16=True, rng=np.random.RandomState(1), graphed=False)
    assert res["n"] == 4
    assert calls == ["cls_tail_vote"]

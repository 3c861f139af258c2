"""-m gpu: voting evaluation of the fine-tuned classifier (engine_finetune.validate_vote / GraphedVoteEval,
P/tools/runner_finetune.py:271-335) on the HIP kernels gm3d_vote_sample and gm3d_cls_tail_vote.

Bars: vote_sample bit-equal to the torch op chain; f32 logits within 1e-5 relative (of the largest magnitude) of the aten
head / the reference fixture; predictions and accuracy exact once the recorded top-2 margins show they are decided.
bf16 (the stack output in bf16, the head in f32 from it): 5e-2 relative against the autocast aten head -- the same bar the
fine-tune tests put on bf16 logits (test_gpu_finetune.test_bf16_step_trains), since both sides round their inputs and
weights to bf16 (2^-9 relative each) before 768- and 256-term dot products -- and predictions equal to the fp32 ones on every
cloud whose fp32 margin exceeds twice that bar (0.1 x the largest |logit|)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import model_ref as R
from tests import clouds
from tests.test_gpu_model import rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CFG = dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64, encoder_dims=384)
BF16_BAR = 5e-2


def build(seed=5, drop_path=0.1, cls_dim=40):
    from gm3d_amd.point_transformer import PointTransformer
    torch.manual_seed(0)
    m = PointTransformer(dict(CFG, drop_path_rate=drop_path, cls_dim=cls_dim))
    R.det_fill_(m, seed=seed)
    return m.cuda()


def loader_of(fx):
    return [(None, None, (torch.from_numpy(fx["pts%d" % i]), torch.from_numpy(fx["labels%d" % i]))) for i in range(3)]


def reference_votes(model, points, subsets, scale, shift, point_all):
    """The reference's loop structure (runner_finetune.py:293-305): per vote index_select + gather_operation, per cloud
    pc*xyz1 + xyz2, then model(points) over B clouds.  -> (V,B,cls)."""
    from gm3d_amd import ops
    fps_idx = ops.furthest_point_sample(points, point_all)
    out = []
    for v in range(subsets.size(0)):
        idx = fps_idx.index_select(1, subsets[v]).contiguous()
        pts = ops.gather_operation(points.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        for b in range(points.size(0)):
            pts[b, :, 0:3] = torch.mul(pts[b, :, 0:3], scale[v, b]) + shift[v, b]
        out.append(model(pts))
    return torch.stack(out)


def device_draws(rng, point_all, npoints, times, B):
    from gm3d_amd import engine_finetune as EF
    return [torch.from_numpy(a).cuda() for a in EF.draw_votes(rng, point_all, npoints, times, B)]


@pytest.mark.parametrize("B,N0,npoints,V", [(4, 2048, 1024, 10), (3, 1100, 1024, 2), (2, 8192, 4096, 3), (5, 8192, 8192, 1)])
def test_vote_sample_equals_torch_chain(B, N0, npoints, V):
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    pts = clouds.gaussian(B, N0, seed=B * 100 + V).cuda()
    point_all = EF.vote_point_all(npoints, N0)
    subsets, scale, shift = device_draws(np.random.RandomState(V), point_all, npoints, V, B)
    fps_idx = ops.furthest_point_sample(pts, point_all)
    got = ops.vote_sample(pts, fps_idx, subsets, scale, shift)
    want = []
    for v in range(V):
        idx = fps_idx.index_select(1, subsets[v]).contiguous()
        p = ops.gather_operation(pts.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        want.append(p * scale[v].unsqueeze(1) + shift[v].unsqueeze(1))
    assert torch.equal(got, torch.cat(want))


def _head(cls_dim, seed):
    h = nn.Sequential(nn.Linear(768, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
                      nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5), nn.Linear(256, cls_dim))
    return R.det_fill_(h, seed=seed).cuda().eval()


@pytest.mark.parametrize("T", [65, 129])
@pytest.mark.parametrize("cls_dim", [15, 40])
def test_cls_tail_vote_against_aten_head(T, cls_dim):
    from gm3d_amd import ops
    V, B = 10, 6
    head = _head(cls_dim, seed=T + cls_dim)
    g = torch.Generator(device="cuda").manual_seed(T * cls_dim)
    x = torch.randn(V * B, T, 384, device="cuda", generator=g)

    def aten(xx):
        with torch.no_grad():
            return head(torch.cat([xx[:, 0], xx[:, 1:].max(1)[0]], dim=-1)).float().view(V, B, cls_dim)

    for dt in (torch.float32, torch.bfloat16):
        xx = x.to(dt)
        want = aten(xx.float())
        labels = want.mean(0).argmax(-1)
        labels[::2] = (labels[::2] + 1) % cls_dim          # half right, half wrong
        correct = torch.full((1,), 5, dtype=torch.long, device="cuda")
        votes = torch.empty(V, B, cls_dim, device="cuda")
        mean, pred = ops.cls_tail_vote(xx, head, labels, V, correct, votes=votes)
        assert rel(votes, want) <= 1e-5, dt                # f32 head on the same (f32 / bf16-valued) features
        assert rel(mean, want.sum(0) / V) <= 1e-5
        assert torch.equal(pred, mean.argmax(-1))
        assert int(correct) == 5 + int((pred == labels).sum())
        ops.cls_tail_vote(xx, head, labels, V, correct)
        assert int(correct) == 5 + 2 * int((pred == labels).sum())      # += on every call
        if dt == torch.bfloat16:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ac = aten(xx)                              # the aten head as model.forward runs it under autocast
            assert rel(votes, ac) <= BF16_BAR
    # the running statistics are read on every call: change them, the result follows
    head[1].running_var.mul_(2.0)
    mean2, _ = ops.cls_tail_vote(x, head, labels, V, correct)
    assert rel(mean2, aten(x).sum(0) / V) <= 1e-5


def test_validate_vote_against_reference_fixture():
    """fp32: per-vote logits of the reference's own test_vote (recorded by a forward hook) within 1e-5; preds and acc exact."""
    from gm3d_amd import engine_finetune as EF
    fx = np.load(os.path.join(GOLD, "vote_b4.npz"))
    votes_ref = [fx["votes%d" % i] for i in range(3)]
    mx = max(float(np.abs(v).max()) for v in votes_ref)
    assert float(fx["margin"].min()) > 1e-3 * mx          # every decision is 100x wider than the 1e-5 bar
    m = build(seed=5).train()
    np.random.seed(int(fx["seed"]))
    res = EF.validate_vote(m, loader_of(fx), "cuda", npoints=int(fx["npoints"]), times=int(fx["times"]), bf16=False, outputs=True)
    assert m.training                                      # the previous mode is restored
    assert res["n"] == 11
    got = res["votes"]
    o = 0
    for v in votes_ref:
        assert rel(got[:, o:o + v.shape[1]], v) <= 1e-5
        o += v.shape[1]
    assert np.array_equal(res["pred"].cpu().numpy(), fx["pred"])
    assert res["acc_vote"] == float(fx["acc"])
    np.random.seed(int(fx["seed"]))
    assert EF.test_vote(m, loader_of(fx), "cuda", bf16=False, graphed=False) == float(fx["acc"])


def test_bf16_preds_match_fp32_where_decided():
    from gm3d_amd import engine_finetune as EF
    fx = np.load(os.path.join(GOLD, "vote_b4.npz"))
    m = build(seed=5)
    np.random.seed(int(fx["seed"]))
    res = EF.validate_vote(m, loader_of(fx), "cuda", bf16=True, outputs=True)
    mx = max(float(np.abs(fx["votes%d" % i].mean(0)).max()) for i in range(3))
    decided = fx["margin"] > 2 * BF16_BAR * mx
    assert decided.sum() >= 8
    assert np.array_equal(res["pred"].cpu().numpy()[decided], fx["pred"][decided])


def test_graph_equals_eager():
    from gm3d_amd import engine_finetune as EF
    m = build(seed=8)
    loader = [(None, None, (clouds.gaussian(4, 2048, seed=200 + i), torch.tensor([1, 2, 3, 4]) * i % 40)) for i in range(3)]
    loader.append((None, None, (clouds.gaussian(3, 2048, seed=299), torch.tensor([5, 6, 7]))))
    for bf16 in (True, False):
        g = EF.validate_vote(m, loader, "cuda", bf16=bf16, rng=np.random.RandomState(11), graphed=True, outputs=True)
        e = EF.validate_vote(m, loader, "cuda", bf16=bf16, rng=np.random.RandomState(11), graphed=False, outputs=True)
        for k in ("votes", "mean", "pred"):
            assert torch.equal(g[k], e[k]), (bf16, k)
        assert g["acc_vote"] == e["acc_vote"] and g["n"] == e["n"] == 15


def test_graph_outlives_training():
    """Capture, train a few flat-optimizer steps (weights, their bf16 shadows and the head's BN statistics change in place),
    replay: equal to an eager pass on the current parameters.  A capture made before the flat optimizer re-pointed the
    parameters is taken again on its next call."""
    from gm3d_amd import engine_finetune as EF
    m = build(seed=9, drop_path=0.0)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    pts = clouds.gaussian(4, 2048, seed=400)
    labels = torch.tensor([1, 5, 9, 13])
    loader = [(None, None, (pts, labels))]
    early = EF.GraphedVoteEval(m, pts.cuda(), labels.cuda(), bf16=True, rng=np.random.RandomState(3), keep_votes=True)
    opt = EF.build_optimizer(m, lr=1e-3, flat=True, max_norm=10.0)
    ge = EF.GraphedVoteEval(m, pts.cuda(), labels.cuda(), bf16=True, rng=np.random.RandomState(3), keep_votes=True)
    graph = ge.graph
    before = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=ge, outputs=True)
    m.train()
    step = EF.GraphedFinetuneStep(m, nn.CrossEntropyLoss(), opt, clouds.gaussian(8, 2048, seed=401).cuda(),
                                  (torch.arange(8) * 5 % 40).cuda(), npoints=1024, bf16=True, rng=np.random.RandomState(2),
                                  augment=False, warmup_iters=3)
    for i in range(3):
        step(clouds.gaussian(8, 2048, seed=410 + i).cuda(), (torch.arange(8) * 3 % 40).cuda())
    torch.cuda.synchronize()
    after = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=ge, outputs=True)
    assert ge.graph is graph                               # replayed, not captured again
    assert m.training
    eager = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=False, outputs=True)
    assert not torch.equal(before["votes"], after["votes"])
    for k in ("votes", "mean", "pred"):
        assert torch.equal(after[k], eager[k]), k
    late = EF.validate_vote(m, loader, "cuda", rng=np.random.RandomState(5), graphed=early, outputs=True)
    for k in ("votes", "mean", "pred"):
        assert torch.equal(late[k], eager[k]), k


def test_batched_forward_against_reference_structure():
    """V*B clouds in one forward against the reference's V forwards of B through model(points), fp32."""
    from gm3d_amd import engine_finetune as EF
    m = build(seed=5).eval()
    B, V = 8, 10
    pts = clouds.gaussian(B, 8192, seed=500).cuda()
    labels = torch.arange(B).cuda()
    subsets, scale, shift = device_draws(np.random.RandomState(6), 1200, 1024, V, B)
    with torch.no_grad():
        want = reference_votes(m, pts, subsets, scale, shift, 1200)
        votes = torch.empty(V, B, 40, device="cuda")
        mean, pred = EF.vote_batch(m, pts, labels, subsets, scale, shift, 1200, torch.zeros(1, dtype=torch.long, device="cuda"),
                                   bf16=False, votes=votes)
        chunked = torch.empty_like(votes)
        EF.vote_batch(m, pts, labels, subsets, scale, shift, 1200, torch.zeros(1, dtype=torch.long, device="cuda"), bf16=False,
                      max_clouds=24, votes=chunked)
    assert rel(votes, want) <= 1e-5
    assert rel(chunked, want) <= 1e-5
    wm = want.mean(0)
    top2 = wm.topk(2, dim=-1).values
    decided = (top2[:, 0] - top2[:, 1]) > 1e-4 * float(wm.abs().max())
    assert bool(decided.any())
    assert torch.equal(pred[decided], wm.argmax(-1)[decided])

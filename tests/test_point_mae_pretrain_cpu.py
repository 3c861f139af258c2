"""CPU: plain Point-MAE pre-training -- the restatement the GPU tests lean on against the reference's fixture, the optimizer
grouping, the per-epoch schedule, the checkpoint layout and the host-side argument guards of the new entry points."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from tests import point_mae_ref as PR

GOLD = os.path.join(os.path.dirname(__file__), "golden", "point_mae_pretrain_b4.npz")
ONE = ctypes.c_void_p(16)      # never dereferenced: the checks fail (or the empty batch returns) first


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


@pytest.mark.parametrize("case", PR.CASES, ids=[c[0] for c in PR.CASES])
def test_restatement_reproduces_the_reference_fixture(fx, case, monkeypatch):
    """Loss and the six recorded gradients within the 1e-5 relative bar the README states for fp32 parity (gradients: of the
    tensor's largest entry).  The fixture's mask and DropPath draws are replayed; block: the recorded start indices give the
    recorded mask."""
    name, mask_type, loss = case
    torch.manual_seed(0)
    m = R.det_fill_(PR.PointMAERef(loss), seed=41).train()
    pts = torch.from_numpy(fx["pts"])
    mask = torch.from_numpy(fx[name + "/mask"])
    if mask_type == "block":
        assert torch.equal(PR.block_mask(torch.from_numpy(fx[name + "/center"]), fx[name + "/start"], 38), mask)
    monkeypatch.setattr(R, "_droppath_feed", [torch.from_numpy(d) for d in fx[name + "/droppath_masks"]])
    out = m(pts, mask)
    assert R._droppath_feed == []
    ref = float(fx[name + "/loss"])
    print(name, "loss", float(out), "fixture", ref)
    assert abs(float(out) - ref) <= 1e-5 * abs(ref)
    out.backward()
    named = dict(m.named_parameters())
    stride = int(fx["stride"])
    for k in PR.GRADS:
        want = torch.from_numpy(fx[name + "/grad/" + k]).double()
        got = PR.picked(named[k].grad, stride).double()
        err = float((got - want).abs().max() / want.abs().max())
        print(name, k, "rel err", err)
        assert err <= 1e-5, k
        n = float(fx[name + "/gradnorm/" + k])
        assert abs(float(named[k].grad.double().norm()) - n) <= 1e-5 * n, k


def _model(mask_type="rand", loss="cdl2"):
    from gm3d_amd.point_mae import Point_MAE
    torch.manual_seed(0)
    return Point_MAE(PR.config(mask_type, loss))


def test_optimizer_groups_follow_the_reference_rule():
    from gm3d_amd import engine_pretrain_point_mae as EP
    m = _model()
    opt = EP.build_optimizer(m, lr=1e-3, weight_decay=0.05, flat=False)
    no_decay, decay = opt.param_groups
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.05
    want_no, want_yes = [], []
    for name, p in m.named_parameters():          # P/tools/builder.py:40-56, restated directly
        (want_no if (p.ndim == 1 or name.endswith(".bias") or "token" in name) else want_yes).append(p)
    assert [id(p) for p in no_decay["params"]] == [id(p) for p in want_no]
    assert [id(p) for p in decay["params"]] == [id(p) for p in want_yes]
    ids_no = {id(p) for p in no_decay["params"]}
    assert id(m.mask_token) in ids_no
    assert all(id(p) in ids_no for n, p in m.named_parameters() if n.endswith(".bias") or p.ndim == 1)
    assert all(p.ndim > 1 for p in decay["params"])
    # the flat optimizer's split is the same rule (its construction needs a GPU: the rule is checked on its own)
    from gm3d_amd.optim import _split_decay
    d, nd = _split_decay(m)
    assert {id(p) for _, p in nd} == ids_no and {id(p) for _, p in d} == {id(p) for p in want_yes}


def test_cosine_schedule():
    """cosine_lr is timm 0.4.5's CosineLRScheduler as build_opti_sche configures it (no warm-up prefix): warmup_lr_init at t = 0;
    the peak at t = warmup_epochs, which WITHOUT a warm-up prefix is the cosine's own value there -- base_lr times
    (1 + cos(pi * warmup / epochs)) / 2 up to lr_min's share, 0.27 % below base_lr for 10 / 300 -- not base_lr itself; monotone on
    both sides of it; lr_min at t = epochs (the cycle limit) up to rounding."""
    from gm3d_amd.engine_pretrain_point_mae import cosine_lr
    base, E, W, lo = 1e-3, 300, 10, 1e-6
    f = lambda t: cosine_lr(t, base, E, W, lr_min=lo, warmup_lr_init=lo)
    assert f(0) == lo
    peak = lo + 0.5 * (base - lo) * (1 + math.cos(math.pi * W / E))
    assert f(W) == peak and base * (1 + math.cos(math.pi * W / E)) / 2 <= f(W) <= base
    assert abs(f(W) - base) <= base * (1 - math.cos(math.pi * W / E)) / 2
    up = [f(t) for t in range(W + 1)]
    down = [f(t) for t in range(W, E + 1)]
    assert all(a < b for a, b in zip(up, up[1:])) and all(a > b for a, b in zip(down, down[1:]))
    assert 0.0 <= f(E) - lo <= 1e-12 and f(E - 1) > lo
    assert f(E + 5) == lo


def test_checkpoint_round_trip(tmp_path):
    from gm3d_amd import checkpoint as C
    from gm3d_amd import engine_pretrain_point_mae as EP
    from gm3d_amd.point_mae import Point_MAE
    from gm3d_amd.point_transformer import PointTransformer
    m = R.det_fill_(_model(), seed=3)
    opt = EP.build_optimizer(m, flat=False)
    path = EP.save_checkpoint(str(tmp_path / "ckpt-last.pth"), m, opt, epoch=7, metrics={"acc": 12.5}, best_metrics={"acc": 13.0})
    ck = C.read_checkpoint(path)
    assert sorted(ck) == ["base_model", "best_metrics", "epoch", "metrics", "optimizer"]
    assert ck["epoch"] == 7 and ck["metrics"] == {"acc": 12.5} and ck["best_metrics"] == {"acc": 13.0}
    assert list(ck["base_model"]) == list(m.state_dict())
    fresh = EP.load_teacher(path, Point_MAE(PR.config()))
    assert not fresh.training and not any(p.requires_grad for p in fresh.parameters())
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), m.state_dict().values()))
    cls = PointTransformer(dict(trans_dim=384, depth=12, drop_path_rate=0.1, cls_dim=40, num_heads=6, group_size=32, num_group=64,
                                encoder_dims=384))
    cls.load_model_from_ckpt(path, key="base_model")
    own = cls.state_dict()
    enc = {k[len("MAE_encoder."):]: v for k, v in m.state_dict().items() if k.startswith("MAE_encoder.")}
    hit = [k for k in enc if k in own]
    assert any(k.startswith("blocks.") for k in hit) and any(k.startswith("encoder.") for k in hit) and any(k.startswith("pos_embed.") for k in hit)
    assert all(torch.equal(own[k], enc[k]) for k in hit)


# ---- argument guards: everything below returns on the host, before any launch
def _mc(G=64, num_mask=38, B=1, mode=0, keys=ONE, start=None, mask=ONE, order=ONE, pitch=None):
    from gm3d_amd._capi import lib
    return lib.gm3d_mask_centers(keys, start, mode, B, G, num_mask, mask, order, G if pitch is None else pitch, None)


def _l1_fwd(B=1, M=38, T=64, **null):
    from gm3d_amd._capi import lib
    a = dict(pred=ONE, target=ONE, ids=ONE, matrix=ONE, i1=ONE, i2=ONE, mean=ONE)
    a.update(null)
    return lib.gm3d_patch_chamfer_l1_loss_fwd(a["pred"], M * 96, a["target"], a["ids"], M, B, T, M, a["matrix"], a["i1"], a["i2"],
                                              a["mean"], 0, None)


def _l1_bwd(B=1, M=38, T=64, **null):
    from gm3d_amd._capi import lib
    a = dict(pred=ONE, target=ONE, ids=ONE, i1=ONE, i2=ONE, g=ONE, dpred=ONE)
    a.update(null)
    return lib.gm3d_patch_chamfer_l1_loss_bwd(a["pred"], M * 96, a["target"], a["ids"], M, a["i1"], a["i2"], a["g"], B, T, M,
                                              a["dpred"], 0, None)


GUARDS = [
    ("mask_centers.G=513", lambda: _mc(G=513, num_mask=300), "EUNSUPPORTED"),
    ("mask_centers.G=512.B=0", lambda: _mc(G=512, num_mask=307, B=0), "OK"),
    ("mask_centers.G=0", lambda: _mc(G=0, num_mask=0), "EINVAL"),
    ("mask_centers.num_mask=G", lambda: _mc(G=64, num_mask=64), "EINVAL"),
    ("mask_centers.num_mask=-1", lambda: _mc(G=64, num_mask=-1), "EINVAL"),
    ("mask_centers.keys=NULL", lambda: _mc(keys=None), "EINVAL"),
    ("mask_centers.mask=NULL", lambda: _mc(mask=None), "EINVAL"),
    ("mask_centers.order=NULL", lambda: _mc(order=None), "EINVAL"),
    ("mask_centers.block.start=NULL", lambda: _mc(mode=1, start=None), "EINVAL"),
    ("mask_centers.block.B=0", lambda: _mc(mode=1, start=ONE, B=0), "OK"),
    ("mask_centers.mode=2", lambda: _mc(mode=2, start=ONE), "EINVAL"),
    ("mask_centers.id_pitch<G", lambda: _mc(pitch=63), "EINVAL"),
    ("mask_centers.B=0", lambda: _mc(B=0), "OK"),
    ("l1_fwd.B=0", lambda: _l1_fwd(B=0), "OK"),
    ("l1_bwd.B=0", lambda: _l1_bwd(B=0), "OK"),
    ("l1_fwd.M>T", lambda: _l1_fwd(M=65, T=64), "EINVAL"),
    ("l1_bwd.M>T", lambda: _l1_bwd(M=65, T=64), "EINVAL"),
    ("l1_fwd.M=0", lambda: _l1_fwd(M=0), "EINVAL"),
    ("l1_fwd.B*M", lambda: _l1_fwd(B=1 << 21, M=32, T=64), "EUNSUPPORTED"),
] + [("l1_fwd.%s=NULL" % k, (lambda k=k: _l1_fwd(**{k: None})), "EINVAL") for k in ("pred", "target", "ids", "matrix", "i1", "i2", "mean")] \
  + [("l1_bwd.%s=NULL" % k, (lambda k=k: _l1_bwd(**{k: None})), "EINVAL") for k in ("pred", "target", "ids", "i1", "i2", "g", "dpred")]


@pytest.mark.parametrize("row", GUARDS, ids=[r[0] for r in GUARDS])
def test_argument_guards_answer_before_any_launch(row):
    from gm3d_amd import _capi
    assert row[1]() == getattr(_capi, "GM3D_" + row[2]), row[0]


def test_header_states_the_mask_limits_in_words():
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gm3d.h")).read()
    assert "1 <= G <= 512" in txt and "0 <= num_mask < G" in txt

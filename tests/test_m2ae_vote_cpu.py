"""CPU: the argument checks of gm3d_cls_tail_vote_pool (the Point-M2AE classifiers' vote tail) and of its Python and engine layers
(no compute calls here).  Every refused value returns before any launch: the pointers are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

ONE = ctypes.c_void_p(16)      # never dereferenced: the checks fail first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pool(x=ONE, V=10, B=4, T=64, C=384, mode=0, cls_dim=40, heads=None, labels=ONE, mean=ONE, pred=ONE, correct=ONE, dtype=0):
    from gm3d_amd._capi import lib
    hp = heads if heads is not None else [ONE] * 14
    return lib.gm3d_cls_tail_vote_pool(x, V, B, T, C, mode, *hp, cls_dim, 1e-5, labels, mean, pred, correct, None, None, dtype, None)


# (parameter, last accepted, first refused).  With B = 0 the entry point returns GM3D_OK right after its shape checks, launching
# nothing: the accepted side passes the guard without a GPU, the refused side is refused by it.
LIMITS = [("T", 512, 513), ("V", 16, 17), ("cls_dim", 256, 257), ("mode", 1, 2)]


@pytest.mark.parametrize("name,ok,refused", LIMITS, ids=[r[0] for r in LIMITS])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_limit_edges(name, ok, refused, dtype):
    from gm3d_amd._capi import GM3D_OK, GM3D_EUNSUPPORTED
    assert _pool(**{name: ok, "B": 0, "dtype": dtype}) == GM3D_OK
    assert _pool(**{name: refused, "B": 0, "dtype": dtype}) == GM3D_EUNSUPPORTED
    assert _pool(**{name: refused, "B": 4, "dtype": dtype}) == GM3D_EUNSUPPORTED


def test_refused_before_any_launch():
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_EUNSUPPORTED, GM3D_BF16
    assert _pool(x=None, B=4) == GM3D_EINVAL
    for i in range(14):
        assert _pool(heads=[ONE] * i + [None] + [ONE] * (13 - i), B=4) == GM3D_EINVAL, i
    assert _pool(labels=None, B=4) == GM3D_EINVAL and _pool(mean=None, B=4) == GM3D_EINVAL
    assert _pool(pred=None, B=4) == GM3D_EINVAL and _pool(correct=None, B=4) == GM3D_EINVAL
    for kw in ({"V": 0}, {"T": 0}, {"cls_dim": 0}, {"B": -1}):
        assert _pool(**dict({"B": 4}, **kw)) == GM3D_EINVAL, kw
    assert _pool(mode=-1, B=4) == GM3D_EUNSUPPORTED and _pool(mode=2, B=4) == GM3D_EUNSUPPORTED
    assert _pool(C=256, B=4) == GM3D_EUNSUPPORTED and _pool(C=768, B=4) == GM3D_EUNSUPPORTED
    assert _pool(dtype=7, B=4) == GM3D_EUNSUPPORTED
    assert _pool(x=ctypes.c_void_p(24), B=4, dtype=GM3D_BF16) == GM3D_EUNSUPPORTED     # rows are read 16 bytes at a time
    assert _pool(x=ctypes.c_void_p(40), B=4) == GM3D_EUNSUPPORTED


def test_header_states_the_table():
    txt = open(os.path.join(ROOT, "include", "gm3d.h")).read()
    i = txt.index("gm3d_cls_tail_vote_pool:")
    limits = re.search(r"Limits: (.*?)\*/", txt[i:], flags=re.S).group(1)
    lim = dict((r[0], r[1]) for r in LIMITS)
    assert "C == 384" in limits
    assert "1 <= T <= %d" % lim["T"] in limits
    assert "1 <= V <= %d" % lim["V"] in limits
    assert "1 <= cls_dim <= %d" % lim["cls_dim"] in limits
    assert "mode 0 or %d" % lim["mode"] in limits
    assert "B == 0 returns GM3D_OK after the shape checks" in txt[i:]


def _head(F_in, cls_dim=40):
    return nn.Sequential(nn.Linear(F_in, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5),
                         nn.Linear(256, 256), nn.BatchNorm1d(256), nn.ReLU(inplace=True), nn.Dropout(0.5), nn.Linear(256, cls_dim))


def test_op_refuses_cpu_tensors_and_a_head_of_the_wrong_width(monkeypatch):
    from gm3d_amd import ops
    launched = []
    monkeypatch.setattr(ops, "_launch", lambda *a, **k: launched.append(a))
    labels, correct = torch.zeros(4, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    with pytest.raises(RuntimeError):
        ops.cls_tail_vote_pool(torch.zeros(40, 64, 384), _head(384), 0, labels, 10, correct)
    # the head's width is checked against the mode before any launch (here: before the device checks of the head can pass)
    monkeypatch.setattr(ops, "_require", lambda *a, **k: None)
    for mode, F_in in ((0, 768), (1, 384)):
        with pytest.raises(RuntimeError, match="input width"):
            ops.cls_tail_vote_pool(torch.zeros(40, 64, 384), _head(F_in), mode, labels, 10, correct)
    with pytest.raises(RuntimeError, match="pool mode"):
        ops.cls_tail_vote_pool(torch.zeros(40, 64, 384), _head(384), 2, labels, 10, correct)
    assert not launched


class _Other(nn.Module):
    cls_dim = 40

    def __init__(self):
        super().__init__()
        self.cls_head_finetune = _head(768)

    def forward_tokens(self, pts):
        raise AssertionError("forward_tokens must not run")


def test_unsupported_model_raises_type_error_before_any_launch(monkeypatch):
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    calls = []
    for name in ("furthest_point_sample", "vote_sample", "cls_tail_vote", "cls_tail_vote_pool"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: calls.append(_n))
    m = _Other().train()
    pts, labels = torch.zeros(2, 2048, 3), torch.zeros(2, dtype=torch.long)
    with pytest.raises(TypeError):
        EF.vote_batch(m, pts, labels, torch.zeros(10, 1024, dtype=torch.long), torch.ones(10, 2, 3), torch.zeros(10, 2, 3), 1200,
                      torch.zeros(1, dtype=torch.long))
    loader = [(None, None, (pts, labels))]
    for graphed in (True, False):
        with pytest.raises(TypeError):
            EF.validate_vote(m, loader, "cpu", graphed=graphed)
        assert m.training
    with pytest.raises(TypeError):
        EF.test_vote(m, loader, "cpu")
    assert not calls


def test_vote_tail_dispatch():
    """PointTransformer keeps cls_tail_vote; each Point-M2AE classifier gets cls_tail_vote_pool with its own pool mode."""
    from gm3d_amd import engine_finetune as EF
    from gm3d_amd import ops
    from gm3d_amd import point_m2ae_cls as C
    from gm3d_amd.point_transformer import PointTransformer
    seen = []
    orig = (ops.cls_tail_vote, ops.cls_tail_vote_pool)
    try:
        ops.cls_tail_vote = lambda x, head, labels, V, correct, votes=None: seen.append(("mae", head, None))
        ops.cls_tail_vote_pool = lambda x, head, mode, labels, V, correct, votes=None: seen.append(("m2ae", head, mode))
        pt = PointTransformer(dict(trans_dim=384, depth=1, drop_path_rate=0.0, cls_dim=40, num_heads=6, group_size=32,
                                   num_group=64, encoder_dims=384))
        mn = C.build_model(dict(NAME="Point_M2AE_ModelNet40", cls_dim=40, encoder_depths=[1, 1, 1]))
        so = C.build_model(dict(NAME="Point_M2AE_ScanObjectNN", cls_dim=15, encoder_depths=[1, 1, 1]))
        for m in (pt, mn, so):
            EF.vote_tail(m)(None, None, 10, None)
    finally:
        ops.cls_tail_vote, ops.cls_tail_vote_pool = orig
    assert seen == [("mae", pt.cls_head_finetune, None), ("m2ae", mn.cls_head_finetune, 0), ("m2ae", so.cls_head_finetune, 1)]

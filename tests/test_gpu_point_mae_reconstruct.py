"""-m gpu: the reconstruction pass -- gm3d_reconstruct_assemble against the aten chain it replaces (bit for bit), Point_MAE(vis=True)
against the reference's own output (tests/golden/reconstruct.npz), reconstruct() / reconstruct_geomask() / runner.test against the
pieces they are made of, one hipGraph capture, and every new allocation under poison.

This module runs before tests/test_gpu_poison_ops.py / _steps.py (alphabetical order): the allocation lines it reaches under poison
stay recorded in poison.SITES and count for their coverage condition."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from oracle import ops as O
from tests import clouds
from tests import point_mae_ref as PR
from tests.test_gpu_model import rel

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = (("rand_b1", "rand"), ("rand_b2", "rand"), ("block_b2", "block"))
K, G, NUM_MASK = 32, 64, 38


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "reconstruct.npz"))


@pytest.fixture(scope="module")
def models():
    """the fixture's model (det_fill_ seed 41), one per mask type, in eval mode; built once"""
    from gm3d_amd.point_mae import Point_MAE
    out = {}
    for mask_type in ("rand", "block"):
        torch.manual_seed(0)
        out[mask_type] = R.det_fill_(Point_MAE(PR.config(mask_type, "cdl2")), seed=41).cuda().eval()
    return out


def _take(x, ids):
    from gm3d_amd.models_mae_learn_loss import take
    return take(x, ids)


def aten_chain(pred, neighborhood, center, vis_ids, mask_ids, flat):
    """P/models/Point_MAE.py:429-437 on id lists instead of boolean masks, and the per-cloud order next to it"""
    B, G_, k, _ = neighborhood.shape
    M = mask_ids.shape[1]
    c_vis, c_mask = _take(center, vis_ids), _take(center, mask_ids)
    full_vis = _take(neighborhood, vis_ids) + c_vis.unsqueeze(2)
    full_rebuild = pred.float().reshape(B, M, k, 3) + c_mask.unsqueeze(2)
    if flat:
        return (torch.cat([full_vis.reshape(-1, 3), full_rebuild.reshape(-1, 3)], dim=0),
                torch.cat([c_mask.reshape(-1, 3), c_vis.reshape(-1, 3)], dim=0))
    return torch.cat([full_vis, full_rebuild], dim=1).reshape(-1, 3), torch.cat([c_vis, c_mask], dim=1).reshape(-1, 3)


def launch(pred, neighborhood, center, vis_ids, mask_ids, layout):
    """the C entry point itself, both outputs pre-filled with NaN"""
    from gm3d_amd._capi import GM3D_BF16, GM3D_F32, check, lib
    from gm3d_amd.ops import _ptr, _stream
    B, G_, k, _ = neighborhood.shape
    V, M = vis_ids.shape[1], mask_ids.shape[1]
    dense = torch.full((B * G_ * k, 3), float("nan"), device="cuda")
    fc = torch.full((B * G_, 3), float("nan"), device="cuda")
    check(lib.gm3d_reconstruct_assemble(_ptr(pred) if M else None, pred.stride(0) if M else 0, _ptr(neighborhood), _ptr(center),
                                        _ptr(vis_ids) if V else None, vis_ids.stride(0) if V else 0, _ptr(mask_ids) if M else None,
                                        mask_ids.stride(0) if M else 0, B, G_, k, V, M, layout, _ptr(dense), _ptr(fc),
                                        GM3D_BF16 if pred.dtype == torch.bfloat16 else GM3D_F32, _stream()), "reconstruct_assemble")
    return dense, fc


def _inputs(B, G_, k, V, M, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    neighborhood = (torch.randn(B, G_, k, 3, generator=g) * 0.1).cuda()
    center = torch.randn(B, G_, 3, generator=g).cuda()
    pred = (torch.randn(B, M, 3 * k, generator=g) * 0.1).cuda().to(dtype)
    order = torch.stack([torch.randperm(G_, generator=g) for _ in range(B)]).cuda()
    return pred, neighborhood, center, order[:, :V].contiguous(), order[:, V:].contiguous()


# --------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("shape", [(1, 64, 32, 26, 38), (3, 5, 1, 2, 3), (2, 7, 5, 0, 7), (2, 7, 5, 7, 0), (2, 6, 33, 2, 4)], ids=str)
def test_assemble_equals_the_aten_chain(shape, layout, dtype):
    """16-byte path (k = 32), scalar path (k = 1, 5, 33), nothing visible, nothing masked, several clouds: every element of both
    NaN-filled outputs is written and equals the aten chain bit for bit."""
    from gm3d_amd import ops
    B, G_, k, V, M = shape
    pred, neighborhood, center, vis_ids, mask_ids = _inputs(B, G_, k, V, M, dtype, seed=sum(shape) + layout)
    dense, fc = launch(pred, neighborhood, center, vis_ids, mask_ids, layout)
    want_dense, want_fc = aten_chain(pred, neighborhood, center, vis_ids, mask_ids, bool(layout))
    assert tuple(dense.shape) == (B * G_ * k, 3) and tuple(fc.shape) == (B * G_, 3)
    assert torch.equal(dense, want_dense), int((dense != want_dense).sum())
    assert torch.equal(fc, want_fc)
    d2, f2 = ops.reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=bool(layout))
    assert torch.equal(d2, dense) and torch.equal(f2, fc) and not d2.requires_grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1])
def test_assemble_takes_strided_views(layout, dtype):
    """pred = the last-M view of a (B,64,96) pix_pred, the id lists = the two column slices of gm3d_mask_centers' (B,64) order:
    nothing is copied, the result is the aten chain's."""
    from gm3d_amd import heads, ops
    B, V, M = 2, G - NUM_MASK, NUM_MASK
    _, neighborhood, center, _, _ = _inputs(B, G, K, V, M, dtype, seed=77 + layout)
    g = torch.Generator().manual_seed(5)
    pix = (torch.randn(B, G, 3 * K, generator=g) * 0.1).cuda().to(dtype)
    _, order = heads.mask_centers(torch.rand(B, G, generator=g).cuda(), M)
    pred, vis_ids, mask_ids = pix[:, -M:], order[:, :V], order[:, V:]
    assert not pred.is_contiguous() and not vis_ids.is_contiguous() and not mask_ids.is_contiguous()
    dense, fc = launch(pred, neighborhood, center, vis_ids, mask_ids, layout)
    want_dense, want_fc = aten_chain(pred, neighborhood, center, vis_ids, mask_ids, bool(layout))
    assert torch.equal(dense, want_dense) and torch.equal(fc, want_fc)
    d2, f2 = ops.reconstruct_assemble(pred, neighborhood, center, vis_ids, mask_ids, flat=bool(layout))
    assert torch.equal(d2, dense) and torch.equal(f2, fc)


# --------------------------------------------------------------------------- Point_MAE(vis=True) against the reference
def _case(fx, name):
    B = fx[name + "/mask"].shape[0]
    pts = torch.from_numpy(fx["pts"][:B]).cuda()
    mask = torch.from_numpy(fx[name + "/mask"]).cuda()
    return pts, mask, B, B * (G - NUM_MASK) * K


@pytest.mark.parametrize("name,mask_type", CASES, ids=[c[0] for c in CASES])
def test_vis_fp32_against_the_reference_fixture(fx, models, name, mask_type):
    """The reference's triple in the reference's shapes.  FPS and KNN are bit-exact and the rest of a visible row is one subtract
    and one add: the visible rows of ret1, all of ret2 and full_center equal the fixture bit for bit.  The rebuilt rows and the
    loss (a second call, vis=False) are within the project's 1e-5."""
    m = models[mask_type]
    pts, mask, B, nv = _case(fx, name)
    with torch.no_grad():
        ret1, ret2, full_center = m(pts.clone(), vis=True, mask=mask)
        loss = m(pts.clone(), mask=mask)
    assert tuple(ret1.shape) == (1, B * G * K, 3) and tuple(ret2.shape) == (1, nv, 3) and tuple(full_center.shape) == (B * G, 3)
    assert ret2.data_ptr() == ret1.data_ptr() and ret2.untyped_storage().data_ptr() == ret1.untyped_storage().data_ptr()
    assert not ret1.requires_grad and not full_center.requires_grad
    want2, want_reb = torch.from_numpy(fx[name + "/ret2"]).cuda(), torch.from_numpy(fx[name + "/rebuilt"]).cuda()
    assert torch.equal(ret2[0], want2) and torch.equal(ret1[0, :nv], want2)
    assert torch.equal(full_center, torch.from_numpy(fx[name + "/full_center"]).cuda())
    err = rel(ret1[0, nv:], want_reb)
    ref = float(fx[name + "/loss"])
    print(name, "rebuilt rel err", err, "loss", float(loss), "fixture", ref, "rel", abs(float(loss) - ref) / abs(ref))
    assert err <= 1e-5
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref)


def test_vis_with_grad_enabled_and_through_mask_noise(fx, models):
    """vis=True outside no_grad returns detached tensors; a noise that ranks exactly the masked groups first (the device path of
    select) gives the bits of mask=."""
    m = models["rand"]
    pts, mask, B, nv = _case(fx, "rand_b2")
    a = m(pts.clone(), vis=True, mask=mask)
    b = m(pts.clone(), vis=True, mask_noise=torch.where(mask, 0.0, 1.0))
    assert all(not t.requires_grad and t.grad_fn is None for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,mask_type", CASES, ids=[c[0] for c in CASES])
def test_vis_bf16_against_the_reference_fixture(fx, models, name, mask_type):
    """bf16 autocast: the rebuilt rows within MULT x the reference's own bf16-autocast error of the same rows (the rule of
    tests/test_gpu_bf16_parity.py); the visible rows never pass through bf16 and are still equal."""
    from tests.test_gpu_bf16_parity import MULT
    m = models[mask_type]
    pts, mask, B, nv = _case(fx, name)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ret1, ret2, full_center = m(pts.clone(), vis=True, mask=mask)
    assert ret1.dtype == torch.float32
    assert torch.equal(ret2[0], torch.from_numpy(fx[name + "/ret2"]).cuda())
    assert torch.equal(full_center, torch.from_numpy(fx[name + "/full_center"]).cuda())
    err, bar = rel(ret1[0, nv:], fx[name + "/rebuilt"]), MULT * float(fx[name + "/ac_err"])
    print(name, "bf16 rebuilt rel err", err, "bar", bar)
    assert err <= bar


# --------------------------------------------------------------------------- reconstruct()
def _fields(r):
    return {k: getattr(r, k) for k in ("dense", "center", "mask", "vis_ids", "mask_ids", "pred", "patch_loss", "loss", "cd_l2", "cd_l1")}


def test_reconstruct_is_made_of_its_pieces(fx, models):
    """loss = the eval-mode forward's, bit for bit; dense / center = the vis=True output regrouped per cloud; cd_l2 / cd_l1 within
    1e-5 of the oracle's CPU Chamfer between each dense cloud and its input."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import runner
    m = models["rand"].train()
    pts, mask, B, nv = _case(fx, "rand_b2")
    V, M = G - NUM_MASK, NUM_MASK
    r = RC.reconstruct(m, pts, mask=mask)
    assert m.training                                    # the mode is restored
    m.eval()
    with torch.no_grad():
        loss = m(pts.clone(), mask=mask)
        ret1, ret2, fc = m(pts.clone(), vis=True, mask=mask)
    assert torch.equal(r.loss, loss) and r.loss.dim() == 0
    assert tuple(r.dense.shape) == (B, G * K, 3) and r.n_visible == V * K and tuple(r.center.shape) == (B, G, 3)
    dense, vis = runner.split_flat(ret1, ret2, B)
    assert torch.equal(r.dense, dense) and torch.equal(r.visible, vis)
    assert torch.equal(r.center, torch.cat([fc[B * M:].view(B, V, 3), fc[:B * M].view(B, M, 3)], dim=1))
    assert torch.equal(r.mask, mask) and tuple(r.vis_ids.shape) == (B, V) and tuple(r.mask_ids.shape) == (B, M)
    assert bool(torch.gather(mask, 1, r.mask_ids).all()) and not bool(torch.gather(mask, 1, r.vis_ids).any())
    # centre i belongs to rows i*k .. i*k+k-1: a visible patch's first point is its own centre (KNN's nearest neighbour)
    assert torch.equal(r.dense.view(B, G, K, 3)[:, :V, 0], r.center[:, :V])
    assert tuple(r.patch_loss.shape) == (B, M) and abs(float(r.patch_loss.mean()) - float(r.loss)) <= 1e-5 * abs(float(r.loss))
    l2, l1 = O.ChamferDistanceL2(reduction="mean"), O.ChamferDistanceL1()
    for b in range(B):
        a, c = r.dense[b:b + 1].cpu(), pts[b:b + 1].cpu()
        w2, w1 = float(l2(a, c)), float(l1(a, c))
        print("cloud", b, "cd_l2", float(r.cd_l2[b]), "oracle", w2, "cd_l1", float(r.cd_l1[b]), "oracle", w1)
        assert abs(float(r.cd_l2[b]) - w2) <= 1e-5 * abs(w2) and abs(float(r.cd_l1[b]) - w1) <= 1e-5 * abs(w1)
    rb = RC.reconstruct(m, pts, mask=mask, bf16=True)
    assert rb.dense.dtype == torch.float32 and torch.equal(rb.visible, r.visible) and bool(torch.isfinite(rb.dense).all())
    assert not torch.equal(rb.dense, r.dense)          # the rebuilt rows did go through bf16


def _ops_sites(sites):
    from gm3d_amd import ops
    src, first = inspect.getsourcelines(ops.reconstruct_assemble)
    return {s for s in sites if s.startswith("gm3d_amd/ops.py:") and first <= int(s.split(":")[1]) < first + len(src)}


@pytest.mark.parametrize("pattern", ["nan", "+inf", "-inf"])
def test_no_result_depends_on_unwritten_memory(fx, models, pattern, tmp_path):
    """reconstruct(), Point_MAE(vis=True) and runner.test with every `empty` allocation filled with NaN / +inf / -inf
    (tests/poison.py) before a kernel writes it: the same bits as without; every allocation line of ops.reconstruct_assemble,
    gm3d_amd/reconstruct.py and gm3d_amd/runner.py is reached."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import runner
    from tests import poison
    m = models["rand"]
    pts, mask, B, nv = _case(fx, "rand_b2")
    noise = torch.where(mask, 0.0, 1.0)

    def run(tag):
        r = RC.reconstruct(m, pts, mask_noise=noise)
        with torch.no_grad():
            triple = m(pts.clone(), vis=True, mask=mask)
        torch.manual_seed(3)
        m.MAE_encoder.device_mask = True
        try:
            recs = runner.test(m, [(["02691156", "03001627"], ["a", "b"], pts.cpu())], out_dir=str(tmp_path / tag))
        finally:
            m.MAE_encoder.device_mask = False
        files = [np.loadtxt(os.path.join(rec["path"], f), delimiter=";") for rec in recs for f in ("vis.txt", "dense_points.txt")]
        return [t.cpu() for t in list(_fields(r).values()) + list(triple)], files

    want, want_files = run("plain")
    with poison.poisoned(pattern) as ps:
        got, got_files = run("poisoned")
    sites = poison.scan_sites()
    mine = _ops_sites(sites) | {s for s in sites if s.startswith(("gm3d_amd/reconstruct.py:", "gm3d_amd/runner.py:"))}
    assert _ops_sites(sites) and mine <= ps.sites, sorted(mine - ps.sites)
    assert len(want) == len(got) and all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(want, got))
    assert len(want_files) == 4 and all(np.array_equal(a, b) for a, b in zip(want_files, got_files))
    assert all(np.isfinite(a.float().numpy()).all() for a in want)


# --------------------------------------------------------------------------- reconstruct_geomask()
def test_reconstruct_geomask():
    """B = 2: the mask is generate_mask_ids' for the same noise and the teacher's predicted loss; dense is the aten chain on the
    student's own pix_pred, neighborhood, center and ids; patch_loss is forward_loss' matrix."""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import models_mae_learn_loss as M
    from gm3d_amd import reconstruct as RC
    torch.manual_seed(0)
    m = R.det_fill_(M.mae_vit_base_patch16_dec512d8b(), seed=0).cuda().train()
    ema = E.ModelEma(m, 0.999)
    B, V = 2, int(G * (1 - 0.6))          # GeoMask3D keeps int(L * (1 - mask_ratio)) = 25 groups and masks 39
    NM = G - V
    pts = clouds.gaussian(B, 1024, seed=61).cuda()
    noise = torch.rand(B, G, generator=torch.Generator().manual_seed(2)).cuda()
    r = RC.reconstruct_geomask(m, ema, pts, epoch=100, total_epoch=400, mask_ratio=0.6, mask_noise=noise)
    assert m.training
    assert tuple(r.teacher_loss_pred.shape) == (B, G) and tuple(r.loss_pred.shape) == (B, NM)
    _, vis_ids, mask_ids, mask = M.generate_mask_ids(r.teacher_loss_pred, 0.6, True, 100, 400, noise, want_bool=True)
    assert torch.equal(r.mask, mask) and torch.equal(r.vis_ids, vis_ids) and torch.equal(r.mask_ids, mask_ids)
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


# --------------------------------------------------------------------------- capture
def test_reconstruct_replays_from_a_graph(models):
    """reconstruct(model, static_pts, mask_noise=static_noise) captured with torch.cuda.graph: replays with fresh inputs equal the
    eager pass bit for bit.  A host synchronisation inside the pass would fail the capture."""
    from gm3d_amd import reconstruct as RC
    m = models["rand"]
    B = 2
    gen = torch.Generator().manual_seed(9)
    xs = [clouds.gaussian(B, 1024, seed=900 + i).cuda() for i in range(3)]
    ns = [torch.rand(B, G, generator=gen).cuda() for _ in range(3)]
    static_pts, static_noise = xs[0].clone(), ns[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RC.reconstruct(m, static_pts, mask_noise=static_noise)          # warm-up: caches are filled outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = RC.reconstruct(m, static_pts, mask_noise=static_noise)
    masks = []
    for x, n in zip(xs[1:], ns[1:]):
        static_pts.copy_(x)
        static_noise.copy_(n)
        graph.replay()
        got = {k: v.clone() for k, v in _fields(r).items()}
        want = _fields(RC.reconstruct(m, x, mask_noise=n))
        assert all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])]
        assert bool(torch.isfinite(got["dense"]).all())
        masks.append(got["mask"])
    assert not torch.equal(masks[0], masks[1])          # the replays did follow their inputs


# --------------------------------------------------------------------------- the tester
def test_runner_files_equal_reconstruct(models, tmp_path):
    """Four clouds in two batches through runner.test: gt.txt, vis.txt and dense_points.txt read back equal the input and
    reconstruct()'s visible / dense tensors for the same draws."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import runner
    m = models["rand"]
    batches = [clouds.gaussian(2, 1024, seed=40 + i) for i in range(2)]
    loader = [(["02691156", "04379243"], ["a", "b"], batches[0]), (["03001627", "03467517"], ["c", "d"], batches[1])]
    m.MAE_encoder.device_mask = True
    try:
        torch.manual_seed(7)
        recs = runner.test(m, loader, out_dir=str(tmp_path / "vis"))
        torch.manual_seed(7)
        want = [RC.reconstruct(m, b.cuda()) for b in batches]
    finally:
        m.MAE_encoder.device_mask = False
    assert [r["idx"] for r in recs] == [0, 1, 2, 3] and [r["view"] for r in recs] == [(90, 135), (30, 30), (30, -45), (0, 90)]
    assert not torch.equal(want[0].mask[0], want[0].mask[1])
    for rec in recs:
        r, b = want[rec["idx"] // 2], rec["idx"] % 2
        assert os.path.basename(rec["path"]) == "%s_%d" % (rec["taxonomy_id"], rec["idx"])
        read = {f: np.loadtxt(os.path.join(rec["path"], f + ".txt"), delimiter=";").astype(np.float32) for f in ("gt", "vis", "dense_points")}
        assert np.array_equal(read["gt"], batches[rec["idx"] // 2][b].numpy())
        assert np.array_equal(read["vis"], r.visible[b].cpu().numpy())
        assert np.array_equal(read["dense_points"], r.dense[b].cpu().numpy())

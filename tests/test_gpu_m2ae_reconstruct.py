"""-m gpu: the Point-M2AE reconstruction pass -- gm3d_reconstruct_partition against its aten restatement (tests/m2ae_reconstruct_ref.py,
bit for bit), reconstruct_m2ae against the pieces it is made of and against the CPU oracle (oracle/hier_ref.py), one hipGraph capture,
runner.test_m2ae, and every new allocation under poison.

This module runs before tests/test_gpu_poison_ops.py / _steps.py (alphabetical order): the allocation lines it reaches under poison
stay recorded in poison.SITES and count for their coverage condition."""
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import clouds
from tests import m2ae_reconstruct_ref as MR

pytestmark = pytest.mark.gpu
LIMIT = 8192
EPOCH, TOTAL = 100, 300
TENSORS = ("dense", "n_visible", "center", "order", "points0", "n_visible0", "mask", "rec", "per_token", "patch_loss", "loss",
           "loss_pred", "teacher_loss_pred", "cd_l2", "cd_l1", "cd_l2_target", "cd_l1_target")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


# --------------------------------------------------------------------------- the kernel
SHAPES = [(1, 1, 1), (2, 5, 1), (3, 64, 8), (2, 65, 5), (2, 256, 8), (1, 512, 16), (2, 1000, 3), (1, LIMIT, 1), (130, 7, 4)]


def _masks(B, G, g):
    """name -> (B,G) uint8: the mask families of the launch test"""
    out = {"none": torch.zeros(B, G, dtype=torch.uint8), "all": torch.ones(B, G, dtype=torch.uint8)}
    out["alternating"] = (torch.arange(G).view(1, G) + torch.arange(B).view(B, 1)).remainder(2).to(torch.uint8)
    out["last_visible"] = torch.ones(B, G, dtype=torch.uint8)
    out["last_visible"][:, -1] = 0
    out["first_masked"] = torch.zeros(B, G, dtype=torch.uint8)
    out["first_masked"][:, 0] = 1
    # random positions, cloud b with (G // 3 + 3b + 1) % (G + 1) masked tokens: as many different counts as B and G allow
    counts = (G // 3 + 3 * torch.arange(B) + 1).remainder(G + 1)
    rank = torch.argsort(torch.rand(B, G, generator=g), dim=1).argsort(dim=1)
    out["random"] = (rank < counts.view(B, 1)).to(torch.uint8)
    assert len(set(out["random"].sum(1).tolist())) == min(B, (G + 1) // math.gcd(3, G + 1))
    values = torch.tensor([1, 2, 255], dtype=torch.uint8)
    out["bytes"] = (torch.rand(B, G, generator=g) < 0.5).to(torch.uint8) * values[torch.randint(0, 3, (B, G), generator=g)]
    return out


def _launch(pred, neighborhood, center, masked):
    """the C entry point itself, every output pre-filled with NaN / -1"""
    from gm3d_amd._capi import GM3D_BF16, GM3D_F32, check, lib
    from gm3d_amd.ops import _ptr, _stream
    B, G, k, _ = neighborhood.shape
    dense = torch.full((B, G * k, 3), float("nan"), device="cuda")
    fc = torch.full((B, G, 3), float("nan"), device="cuda")
    order = torch.full((B, G), -1, dtype=torch.int32, device="cuda")
    nv = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    dt = GM3D_BF16 if pred is not None and pred.dtype == torch.bfloat16 else GM3D_F32
    check(lib.gm3d_reconstruct_partition(_ptr(pred), _ptr(neighborhood), _ptr(center), _ptr(masked), B, G, k, dt, _ptr(dense), _ptr(fc),
                                         _ptr(order), _ptr(nv), _stream()), "reconstruct_partition")
    return dense, fc, order, nv


def _inputs(B, G, k, kind, seed):
    g = torch.Generator().manual_seed(seed)
    neighborhood = (torch.randn(B, G, k, 3, generator=g) * 0.1).cuda()
    center = torch.randn(B, G, 3, generator=g).cuda()
    pred = None if kind == "none" else (torch.randn(B, G, 3 * k, generator=g) * 0.1).cuda().to(
        torch.bfloat16 if kind == "bf16" else torch.float32)
    return pred, neighborhood, center, g


@pytest.mark.parametrize("kind", ["f32", "bf16", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_partition_equals_the_aten_chain(shape, kind):
    """One token, one past a wave (65), the model's two levels on the 16-byte path, the 4-byte path (k = 1, 3, 5), the token limit,
    more clouds than tokens; nothing / everything / every other token masked, one visible token at the end, one masked at the front,
    a different count per cloud, mask bytes 2 and 255: every element of the four pre-filled outputs is written and equals the aten
    chain bit for bit, through the C entry point and through the op."""
    from gm3d_amd import ops
    B, G, k = shape
    pred, neighborhood, center, g = _inputs(B, G, k, kind, seed=sum(shape))
    for name, masked in _masks(B, G, g).items():
        masked = masked.cuda()
        want = MR.partition(pred, neighborhood, center, masked)
        got = _launch(pred, neighborhood, center, masked)
        for w, a, what in zip(want, got, ("dense", "full_center", "order", "n_visible")):
            assert a.shape == w.shape and a.dtype == w.dtype, (name, what)
            assert torch.equal(a, w), (name, what, int((a != w).sum()))
        assert torch.equal(got[3].long(), (masked == 0).sum(1))
        via_op = ops.reconstruct_partition(pred, neighborhood, center, masked.bool() if name != "bytes" else masked)
        assert all(torch.equal(a, w) and not a.requires_grad for a, w in zip(via_op, want)), name


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_rows_of_visible_tokens_are_never_read(kind):
    """pred rows of visible tokens filled with NaN: dense is finite and what it is with ordinary values there."""
    B, G, k = 2, 256, 8
    pred, neighborhood, center, g = _inputs(B, G, k, kind, seed=11)
    masked = _masks(B, G, g)["random"].cuda()
    assert 0 < int(masked.sum()) < B * G
    want = _launch(pred, neighborhood, center, masked)
    holes = pred.clone()
    holes[masked == 0] = float("nan")
    got = _launch(holes, neighborhood, center, masked)
    assert bool(torch.isfinite(got[0]).all()) and all(torch.equal(a, w) for a, w in zip(got, want))


# --------------------------------------------------------------------------- reconstruct_m2ae()
@pytest.fixture(scope="module")
def env():
    """the configuration of tests/test_gpu_m2ae.py: the default model, DropPath off, name-derived weights (student seed 3, teacher
    seed 4), B = 2 clouds of 2048 points, injected mask noise; built once"""
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import point_m2ae as P
    from oracle import model_ref as R
    model = P.PointM2AE()
    for mod in model.modules():
        if hasattr(mod, "drop_prob"):
            mod.drop_prob = 0.0
    R.det_fill_(model, seed=3)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    ema = E.ModelEma(model, 0.999)
    ema.ema.load_state_dict({k: v.clone() for k, v in R.det_fill_(P.PointM2AE(), seed=4).state_dict().items()})
    pts = clouds.gaussian(2, 2048, seed=20)
    noise = torch.rand(2, 64, generator=torch.Generator().manual_seed(5))
    return {"model": model, "ema": ema, "sd": sd, "pts": pts.cuda(), "pts_cpu": pts, "noise": noise.cuda()}


@pytest.fixture(scope="module")
def recon(env):
    """the fp32 pass, computed once and left unchanged"""
    from gm3d_amd import reconstruct as RC
    return RC.reconstruct_m2ae(env["model"], env["pts"], env["ema"], EPOCH, TOTAL, mask_noise=env["noise"])


def _tensors(r):
    out = {k: getattr(r, k) for k in TENSORS}
    out.update({"masks%d" % i: m for i, m in enumerate(r.masks)})
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_reconstruct_m2ae_is_made_of_its_pieces(env, recon, bf16):
    """mask, rec, loss and patch_loss = pretrain_forward's under no_grad in eval mode on the same grouping and noise, bit for bit;
    per_token = forward_loss's; dense / center / order / n_visible at both levels = the aten chain on those tensors; cd_* =
    cloud_chamfer called directly; the static bound of the visible-first order held."""
    from gm3d_amd import point_m2ae as P
    from gm3d_amd import reconstruct as RC
    model, teacher, pts = env["model"], env["ema"].ema, env["pts"]
    r = recon if not bf16 else RC.reconstruct_m2ae(model, pts, env["ema"], EPOCH, TOTAL, mask_noise=env["noise"], bf16=True)
    was = teacher.training
    assert model.training                                                          # the pass restored the mode
    model.eval()
    teacher.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            _, group, prop = P.group_stage(teacher.group_divider, pts, augment=False)
            want = P.pretrain_forward(model, teacher, pts, EPOCH, TOTAL, mask_noise=env["noise"], group=group, prop=prop)
            masks = P.back_project(want["mask"], group[2])
            lo = model.forward_loss(want["rec"], group[0], group[2], masks)
    finally:
        model.train()
        teacher.train(was)
    B, (G0, G1), (k0, k1) = 2, (512, 256), (16, 8)
    assert torch.equal(r.mask, want["mask"]) and r.mask.dtype == torch.bool and int(r.mask[0].sum()) == 52
    assert len(r.masks) == 3 and all(torch.equal(a, b) for a, b in zip(r.masks, masks))
    assert torch.equal(r.rec, want["rec"]) and tuple(r.rec.shape) == (B, G1, k1, 3)
    assert r.rec.dtype == (torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(r.loss, want["loss_chfr"]) and torch.equal(r.patch_loss, want["matrix"]) and torch.equal(r.loss, lo["Chamfer_mean"])
    assert torch.equal(r.per_token, lo["per_token"]) and tuple(r.per_token.shape) == (B, G1)
    assert torch.equal(r.teacher_loss_pred, want["teacher_loss_pred"].float()) and tuple(r.loss_pred.shape) == (B, 64)
    d1 = MR.partition(want["rec"].reshape(B, G1, 3 * k1), group[0][1], group[1][1], masks[1])
    assert all(torch.equal(a, b) for a, b in zip((r.dense, r.center, r.order, r.n_visible), d1))
    d0 = MR.partition(None, group[0][0], group[1][0], masks[0])
    assert torch.equal(r.points0, d0[0]) and torch.equal(r.n_visible0, d0[3])
    assert tuple(r.dense.shape) == (B, G1 * k1, 3) and tuple(r.points0.shape) == (B, G0 * k0, 3) and r.dense.dtype == torch.float32
    assert torch.equal(r.n_visible.long(), (~masks[1]).sum(1)) and torch.equal(r.n_visible0.long(), (~masks[0]).sum(1))
    assert 0 < int(r.n_visible.min()) and int(r.n_visible.max()) < G1
    for (l2, l1), target in (((r.cd_l2, r.cd_l1), pts), ((r.cd_l2_target, r.cd_l1_target), group[1][0])):
        w2, w1 = RC.cloud_chamfer(r.dense, target)
        assert torch.equal(l2, w2) and torch.equal(l1, w1) and tuple(l2.shape) == (B,) and bool(torch.isfinite(l2).all())
    assert int(r.vis_overflow) == 0
    # every visible level-0 point is an input point of its cloud, and visible(b) is the ragged head of dense
    for b in range(B):
        v0 = r.visible0(b)
        assert v0.shape[0] == int(r.n_visible0[b]) * k0 and r.visible(b).shape[0] == int(r.n_visible[b]) * k1
        assert bool((torch.cdist(v0, pts[b], compute_mode="donot_use_mm_for_euclid_dist").min(dim=1).values <= 1e-6).all())
    assert bool(torch.isfinite(r.dense).all())


def test_reconstruct_m2ae_against_the_oracle(env, recon):
    """fp32, the same mask and grouping: rec and the per-token Chamfer loss against oracle/hier_ref.py::m2ae_forward(training=False)
    within the 2e-5 relative of tests/test_gpu_m2ae.py."""
    from oracle import hier_ref as HR
    from oracle import ops as oracle_ops
    oracle_ops.build()
    with torch.no_grad():
        ref = HR.m2ae_forward(env["sd"], env["pts_cpu"], recon.mask.cpu(), training=False)
        _, _, cd = HR.m2ae_losses(ref["rec"], ref["group"][0], ref["group"][2], ref["masks"])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(recon.masks, ref["masks"]))
    e_rec, e_tok = _rel(recon.rec, ref["rec"]), _rel(recon.per_token, cd)
    print("rec rel err", e_rec, "per_token rel err", e_tok)
    assert e_rec <= 2e-5 and e_tok <= 2e-5


def test_reconstruct_m2ae_without_a_teacher(env, recon):
    """An explicit mask stands in for the teacher; no mask, or one that masks nothing, is refused."""
    from gm3d_amd import reconstruct as RC
    model, pts = env["model"], env["pts"]
    r = RC.reconstruct_m2ae(model, pts, mask=recon.mask)
    assert r.teacher_loss_pred is None and torch.equal(r.mask, recon.mask)
    assert all(torch.equal(a, b) for a, b in zip(r.masks, recon.masks))
    assert torch.equal(r.n_visible, recon.n_visible) and torch.equal(r.order, recon.order) and torch.equal(r.points0, recon.points0)
    nb1, c1 = _level1(env)
    want = MR.partition(r.rec.reshape(2, 256, 24), nb1, c1, r.masks[1])
    assert torch.equal(r.dense, want[0]) and torch.equal(r.center, want[1])
    # the visible-first order without a static bound keeps every row: the same visible tokens, so the same reconstruction band
    assert _rel(r.rec, recon.rec) <= 2e-5 and bool(torch.isfinite(r.cd_l2).all())
    with pytest.raises(ValueError):
        RC.reconstruct_m2ae(model, pts)
    with pytest.raises(ValueError):
        RC.reconstruct_m2ae(model, pts, mask=torch.zeros_like(recon.mask))
    assert model.training


def _level1(env):
    from gm3d_amd import point_m2ae as P
    _, group, _ = P.group_stage(env["model"].group_divider, env["pts"], augment=False)
    return group[0][1], group[1][1]


def test_reconstruct_m2ae_replays_from_a_graph(env):
    """reconstruct_m2ae(model, static_pts, teacher, ..., mask_noise=static_noise) captured into one graph: replays on fresh inputs
    copied into the static tensors equal the eager pass bit for bit.  A host synchronisation inside the pass would fail the capture."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import streams
    model, ema = env["model"], env["ema"]
    B = 2
    gen = torch.Generator().manual_seed(9)
    xs = [clouds.gaussian(B, 2048, seed=900 + i).cuda() for i in range(3)]
    ns = [torch.rand(B, 64, generator=gen).cuda() for _ in range(3)]
    static_pts, static_noise = xs[0].clone(), ns[0].clone()
    streams.warm_up(lambda: RC.reconstruct_m2ae(model, static_pts, ema, EPOCH, TOTAL, mask_noise=static_noise), 1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with streams.capture(graph):
        r = RC.reconstruct_m2ae(model, static_pts, ema, EPOCH, TOTAL, mask_noise=static_noise)
    masks = []
    for x, n in zip(xs[1:], ns[1:]):
        static_pts.copy_(x)
        static_noise.copy_(n)
        graph.replay()
        got = {k: v.clone() for k, v in _tensors(r).items()}
        want = _tensors(RC.reconstruct_m2ae(model, x, ema, EPOCH, TOTAL, mask_noise=n))
        assert all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])]
        assert bool(torch.isfinite(got["dense"]).all())
        masks.append(got["mask"])
    assert not torch.equal(masks[0], masks[1])          # the replays did follow their inputs
    assert int(r.vis_overflow) == 0


# --------------------------------------------------------------------------- poison
def _ops_sites(sites):
    from gm3d_amd import ops
    src, first = inspect.getsourcelines(ops.reconstruct_partition)
    return {s for s in sites if s.startswith("gm3d_amd/ops.py:") and first <= int(s.split(":")[1]) < first + len(src)}


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()


@pytest.mark.parametrize("pattern", ["nan", "+inf", "-inf"])
def test_no_result_depends_on_unwritten_memory(env, pattern, tmp_path):
    """reconstruct_m2ae() and runner.test_m2ae with every `empty` allocation filled with NaN / +inf / -inf (tests/poison.py) before a
    kernel writes it: the same bits as without; every allocation line of ops.reconstruct_partition, gm3d_amd/reconstruct.py and
    gm3d_amd/runner.py is reached."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import runner
    from tests import poison
    model, ema, pts = env["model"], env["ema"], env["pts"]

    def run(tag):
        r = RC.reconstruct_m2ae(model, pts, ema, EPOCH, TOTAL, mask_noise=env["noise"])
        torch.manual_seed(3)
        recs = runner.test_m2ae(model, ema, [(["02691156", "03001627"], ["a", "b"], pts.cpu())], str(tmp_path / tag), EPOCH, TOTAL)
        files = [np.loadtxt(os.path.join(rec["path"], f), delimiter=";") for rec in recs for f in ("vis.txt", "dense_points.txt")]
        return [t.cpu() for t in _tensors(r).values()], files

    want, want_files = run("plain")
    with poison.poisoned(pattern) as ps:
        got, got_files = run("poisoned")
    sites = poison.scan_sites()
    mine = _ops_sites(sites) | {s for s in sites if s.startswith(("gm3d_amd/reconstruct.py:", "gm3d_amd/runner.py:"))}
    assert len(_ops_sites(sites)) == 4 and mine <= ps.sites, sorted(mine - ps.sites)
    assert len(want) == len(got) and all(_bytes(a) == _bytes(b) for a, b in zip(want, got))
    assert len(want_files) == 4 and all(np.array_equal(a, b) for a, b in zip(want_files, got_files))
    assert all(bool(torch.isfinite(a.float()).all()) for a in want)


# --------------------------------------------------------------------------- the tester
def test_runner_m2ae_files_equal_reconstruct_m2ae(env, tmp_path):
    """One batch of two clouds through runner.test_m2ae: gt.txt, vis.txt and dense_points.txt read back equal the input, the ragged
    visible level-0 points and the dense level-1 cloud of reconstruct_m2ae for the same draw."""
    from gm3d_amd import reconstruct as RC
    from gm3d_amd import runner
    model, ema = env["model"], env["ema"]
    batch = clouds.gaussian(2, 2048, seed=40)
    torch.manual_seed(7)
    recs = runner.test_m2ae(model, ema, [(["02691156", "04379243"], ["a", "b"], batch)], str(tmp_path / "vis"), EPOCH, TOTAL)
    torch.manual_seed(7)
    r = RC.reconstruct_m2ae(model, batch.cuda(), ema, EPOCH, TOTAL)
    assert [rec["idx"] for rec in recs] == [0, 1] and [rec["view"] for rec in recs] == [(90, 135), (30, 30)]
    rows = []
    for b, rec in enumerate(recs):
        assert os.path.basename(rec["path"]) == "%s_%d" % (rec["taxonomy_id"], rec["idx"])
        read = {f: np.loadtxt(os.path.join(rec["path"], f + ".txt"), delimiter=";").astype(np.float32) for f in ("gt", "vis", "dense_points")}
        assert np.array_equal(read["gt"], batch[b].numpy())
        assert np.array_equal(read["vis"], r.visible0(b).cpu().numpy())
        assert np.array_equal(read["dense_points"], r.dense[b].cpu().numpy())
        rows.append(read["vis"].shape[0])
    assert all(n % 16 == 0 and 0 < n < 512 * 16 for n in rows)

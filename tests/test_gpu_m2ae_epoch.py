"""-m gpu: Point-M2AE pretraining as a training path -- the grouping stage's own generator (look-ahead no longer changes the random
draws), engine_pretrain_m2ae.train_one_epoch (eager warm-up, then replays; the visible-token overflow guard), checkpoint resume,
the checkpoint feeding the ModelNet40 classifier, and the one-rank SegmentedM2AEStep against its eager form and against the
single-backward pretrain_step.  Small batches (B = 8 clouds of 2048 points), bf16 like the measured configuration."""
from types import SimpleNamespace

import pytest
import torch

from tests import clouds

pytestmark = pytest.mark.gpu
B = 8


def _args(**kw):
    a = dict(bf16=True, epochs=300, lr=1e-3, min_lr=1e-6, warmup_epochs=10, accum_iter=1, seed=0)
    a.update(kw)
    return SimpleNamespace(**a)


def _model(seed, drop_path=True, segmented=False):
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(seed)
    m = P.PointM2AE().cuda().train()
    if not drop_path:
        for mod in m.modules():
            if hasattr(mod, "drop_prob"):
                mod.drop_prob = 0.0
    opt, ema = EM.build_optimizer(m, lr=1e-3, segmented=segmented)
    return m, ema, opt


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def test_own_generator_makes_look_ahead_irrelevant():
    """Augmentation ON, DropPath ON: GraphedM2AEStep with its own augmentation generator, replayed with look-ahead, follows the
    same trajectory -- losses, flat parameters, teacher: equal -- as the same step replayed without look-ahead (4 steps, equal
    seeds).  The two stages' graphs replay on two streams; on one shared generator the replay order decided the draws."""
    from gm3d_amd import point_m2ae as P
    pool = [clouds.gaussian(B, 2048, seed=900 + i).cuda() for i in range(5)]
    args = _args()
    res = []
    for look_ahead in (True, False):
        torch.cuda.manual_seed(77)                  # the training graph's draws (DropPath, mask noise): the same sequence per twin
        m, ema, opt = _model(31)
        step = P.GraphedM2AEStep(m, ema, opt, args, pool[0], 100, warmup_iters=1, generator=_gen(5))
        losses = []
        for i in range(4):
            o = step(pool[i], next_pts=pool[i + 1] if look_ahead else None)
            losses.append([float(o[k]) for k in ("loss_chfr", "loss_learn", "grad_norm")])
        torch.cuda.synchronize()
        res.append((losses, opt.P.clone(), opt.E.clone()))
        del step, m, ema, opt
    (la, pa, ea), (lb, pb, eb) = res
    assert all(x == x for row in la for x in row)
    assert la == lb, (la, lb)
    assert torch.equal(pa, pb) and torch.equal(ea, eb)


def test_train_one_epoch_warms_up_then_replays():
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd import engine_pretrain_m2ae as EM
    m, ema, opt = _model(3)
    loader = [clouds.gaussian(B, 2048, seed=40 + i) for i in range(5)]      # CPU batches: the engine moves them
    args = _args()
    s0 = EM.train_one_epoch(m, loader, opt, "cuda", 0, args=args, model_ema=ema, print_freq=2)
    s1 = EM.train_one_epoch(m, loader, opt, "cuda", 1, args=args, model_ema=ema, print_freq=2)
    assert s0["replayed_iters"] == 5 - E.EAGER_WARMUP_ITERS and s0["capture_s"] > 0
    assert s1["replayed_iters"] == 5
    for st in (s0, s1):
        for k in ("loss", "loss_learn", "loss_chfr", "grad_norm", "lr"):
            assert st[k] == st[k] and abs(st[k]) != float("inf"), (k, st)
        assert st["loss_mse"] == 0.0 and st["loss_chfr"] > 0
    assert abs(ema.decay - E.ema_decay_for_epoch(1)) < 1e-12


def test_too_small_visible_bound_raises():
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import masked_stack as S
    m, ema, opt = _model(4, drop_path=False)
    G = m.cfg["num_groups"]
    m._compact_bounds = lambda vis_count: [G[0], 32, 16]      # ~96 visible level-1 tokens per cloud do not fit in 32 rows
    loader = [clouds.gaussian(B, 2048, seed=60 + i) for i in range(2)]
    try:
        with pytest.raises(RuntimeError, match="overflow"):
            EM.train_one_epoch(m, loader, opt, "cuda", 0, args=_args(), model_ema=ema, print_freq=1, use_graph=False)
    finally:
        S.overflow_flag(torch.device("cuda")).zero_()


def _steps(m, ema, opt, data, noise, gen, epoch=100):
    from gm3d_amd import point_m2ae as P
    out = []
    for x, z in zip(data, noise):
        staged = P.group_stage(ema.ema.group_divider, x.clone(), augment=True, generator=gen)
        o = P.pretrain_step(m, ema, opt, None, epoch, _args(), mask_noise=z, staged=staged)
        out.append([float(o[k]) for k in ("loss_chfr", "loss_learn", "grad_norm")])
    torch.cuda.synchronize()
    return out


def test_checkpoint_resume_continues_bit_for_bit(tmp_path):
    from gm3d_amd import checkpoint as C
    from gm3d_amd import point_m2ae_cls as PC
    data = [clouds.gaussian(B, 2048, seed=80 + i).cuda() for i in range(3)]
    noise = [torch.rand(B, 64, generator=torch.Generator().manual_seed(90 + i)).cuda() for i in range(3)]
    m, ema, opt = _model(7, drop_path=False)
    gen = _gen(11)
    _steps(m, ema, opt, data[:1], noise[:1], gen)
    path = str(tmp_path / "ckpt.pth")
    C.save_checkpoint(path, m, opt, epoch=4, model_name="Point_M2AE", model_ema=ema)
    gen_state = gen.get_state()
    want = _steps(m, ema, opt, data[1:], noise[1:], gen)
    p_want, e_want = opt.P.clone(), opt.E.clone()
    bufs_want = [b.clone() for b in m.buffers()]

    m2, ema2, opt2 = _model(8, drop_path=False)                 # another seed: everything has to come from the file
    assert not torch.equal(opt2.P, opt.P)
    start = C.load_checkpoint(path, m2, opt2, model_ema=ema2)
    assert start == 5
    ema2.decay = ema.decay
    gen2 = _gen(0)
    gen2.set_state(gen_state)
    got = _steps(m2, ema2, opt2, data[1:], noise[1:], gen2)
    assert got == want, (got, want)
    assert torch.equal(opt2.P, p_want) and torch.equal(opt2.E, e_want)
    assert all(torch.equal(a, b) for a, b in zip(m2.buffers(), bufs_want))

    # the file feeds the ModelNet40 classifier: every encoder key present
    cls = PC.Point_M2AE_ModelNet40(dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64],
                                        encoder_depths=[5, 5, 5], encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28],
                                        drop_path_rate=0.1, num_heads=6, cls_dim=40))
    for key in ("state_dict", "ema_state_dict"):
        r = cls.load_pretrained_state(C.read_checkpoint(path)[key])
        assert all(k.startswith("cls_head_finetune.") for k in r.missing_keys), r.missing_keys
        assert torch.equal(cls.encoder_blocks[2].blocks[0].mlp.fc1.weight, C.read_checkpoint(path)[key]["encoder_blocks.2.blocks.0.mlp.fc1.weight"])


def test_one_rank_segmented_step_equals_its_eager_form_and_the_single_backward():
    """SegmentedM2AEStep without a process group: (1) the captured six graphs follow the eager segments' trajectory bit for bit over
    3 steps; (2) the flat gradient of the four segments matches pretrain_step's single backward.  (2) allows 1e-5 of each
    parameter's largest gradient: a segment's deferred weight gradients form their own one-launch batch, and the NT kernel's default
    row splits -- the fp32 summation order of a weight gradient -- depend on the whole launch's composition (gemm.wgrad_nt_multi);
    the sum at the enc[1] cut is the one the single backward forms (a + b in the activation type)."""
    from gm3d_amd import wgrads
    from gm3d_amd import point_m2ae as P
    data = [clouds.gaussian(B, 2048, seed=120 + i).cuda() for i in range(4)]
    noise = [torch.rand(B, 64, generator=torch.Generator().manual_seed(130 + i)).cuda() for i in range(4)]
    args = _args()
    traj = {}
    for graphs in (False, True):
        m, ema, opt = _model(9, drop_path=False, segmented=True)
        # one eager iteration on both twins: what the engine runs before a capture
        P.SegmentedM2AEStep(m, ema, opt, args, data[0], 100, augment=False, inject_mask_noise=True, use_graphs=False)(data[0], noise[0])
        step = P.SegmentedM2AEStep(m, ema, opt, args, data[0], 100, augment=False, inject_mask_noise=True, warmup_iters=0,
                                   use_graphs=graphs, broadcast=False)
        losses = []
        for i in range(1, 4):
            o = step(data[i], mask_noise=noise[i])
            losses.append([float(o[k]) for k in ("loss_chfr", "loss_learn", "grad_norm")])
        torch.cuda.synchronize()
        traj[graphs] = (losses, opt.P.clone(), opt.E.clone())
        del step
    assert traj[True][0] == traj[False][0], traj
    assert torch.equal(traj[True][1], traj[False][1]) and torch.equal(traj[True][2], traj[False][2])

    # (2) one model, one optimizer layout: the single backward's gradient, then the four segments' on the same state and inputs
    m, ema, opt = _model(10, drop_path=False, segmented=True)
    seg = P.SegmentedM2AEStep(m, ema, opt, args, data[0], 100, augment=False, inject_mask_noise=True, use_graphs=False)
    staged = lambda: P.group_stage(ema.ema.group_divider, data[1].clone(), augment=False)
    opt.zero_grad(set_to_none=True)
    pts, group, prop = staged()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = P.pretrain_forward(m, ema.ema, pts, 100, args.epochs, mask_noise=noise[1], group=group, prop=prop)
    with wgrads.async_wgrad(out["loss"].device, defer_heads=True):
        out["loss"].backward()
    opt.gather_grads()
    g_single = opt.G.clone()
    opt.G.zero_()
    seg.static_noise.copy_(noise[1])
    st = staged()
    for k in range(4):
        seg._segment(k, st if k == 0 else None)
    torch.cuda.synchronize()
    g_seg = opt.G.clone()
    assert torch.isfinite(g_seg).all() and g_seg.abs().sum() > 0
    names = [n for n, _ in opt._named]
    offs = list(opt._offs) + [opt.n]
    worst = []
    for n, lo, p in zip(names, offs[:-1], opt._params):
        a, b = g_seg[lo:lo + p.numel()], g_single[lo:lo + p.numel()]
        dev = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        worst.append((dev, n))
    worst.sort(reverse=True)
    assert worst[0][0] <= 1e-5, worst[:5]

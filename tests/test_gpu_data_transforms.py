"""-m gpu: gm3d_augment (gm3d_amd/csrc/augment.hip) through gm3d_amd/data_transforms.py -- the kernel against the reference's
fixture, against the torch restatement at sizes the fixture does not reach, with live draws, inside a captured graph, against the
older gm3d_scale_translate, and inside the captured Point-MAE step.  The bars are tests/test_data_transforms_cpu.py's: torch.equal
everywhere except where a rotation is involved, there 2^-21 of the cloud's largest |coordinate|."""
import pytest
import torch

from tests.test_data_transforms_cpu import CHAINS, OPS, SIZES, case, check, fx, make  # noqa: F401 (fx is a fixture)

pytestmark = pytest.mark.gpu


def chain_a(T):
    return [T.PointcloudScale(), T.PointcloudTranslate(), T.PointcloudJitter(), T.PointcloudRandomInputDropout(), T.RandomHorizontalFlip()]


def every_op(T):
    """all seven, none with its default arguments, the rotation last (the bar is stated for the rotation's own output)"""
    return [T.RandomHorizontalFlip("x"), T.PointcloudScale(0.5, 2.0), T.PointcloudRandomInputDropout(0.5), T.PointcloudTranslate(0.3),
            T.PointcloudJitter(0.02, 0.03), T.PointcloudScaleAndTranslate(0.8, 1.25, 0.1), T.PointcloudRotate()]


def clouds_for(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    pc = (torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.3])
    if B > 1:
        pc[1] += 5.0
    if B > 2:
        pc[2] *= 1e-3
    return pc


def injected(T, chain, B, N, seed):
    """one `draws=` entry per op of the chain, from a CPU generator"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in chain:
        kind = T._spec(t)[0]
        out.append({T.ROTATE: lambda: torch.rand(B, generator=g), T.SCALE: lambda: torch.rand(B, 3, generator=g) + 0.5,
                    T.TRANSLATE: lambda: torch.rand(B, 3, generator=g) - 0.5,
                    T.SCALE_TRANSLATE: lambda: (torch.rand(B, 3, generator=g) + 0.5, torch.rand(B, 3, generator=g) - 0.5),
                    T.JITTER: lambda: torch.randn(B, N, 3, generator=g) * 0.02,
                    T.DROPOUT: lambda: (torch.rand(B, generator=g) * 0.5, torch.rand(B, N, generator=g)),
                    T.FLIP: lambda: torch.rand(B, 3, generator=g)}[kind]())
    return out


# ------------------------------------------------------------------------------------------------ (a) against the reference
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("what", OPS + tuple(CHAINS))
def test_kernel_equals_reference(fx, N, what):
    from gm3d_amd import data_transforms as T
    names, pc, draws, want = case(fx, N, what)
    x = pc.cuda()
    out = T.Compose([make(n) for n in names])(x, draws=draws)
    assert out is x
    check(x.cpu().numpy(), want, names, "kernel")


# ------------------------------------------------------------------------------------------------ (b) against the restatement
@pytest.mark.parametrize("B,N", [(3, 8192), (2, 1500)])
def test_kernel_equals_fallback_on_injected_draws(B, N):
    """8192: eight points per thread, sixteen waves; 1500: threads with one point and threads with two"""
    from gm3d_amd import data_transforms as T
    pc = clouds_for(B, N, N)
    singles = [[t] for t in every_op(T)]
    for i, chain in enumerate(singles + [chain_a(T), every_op(T)]):
        draws = injected(T, chain, B, N, 100 * N + i)
        want = T.Compose(chain)(pc.clone(), draws=draws)                   # CPU: the restatement
        got = T.Compose(chain)(pc.cuda(), draws=draws)                     # the kernel
        names = ["rotate" if T._spec(t)[0] == T.ROTATE else type(t).__name__ for t in chain]
        assert not torch.equal(want, pc)
        check(got.cpu().numpy(), want.numpy(), names, "N=%d" % N)


# ------------------------------------------------------------------------------------------------ (c) live draws
@pytest.mark.parametrize("which", ["chainA", "every_op"])
def test_live_draws_equal_fallback_on_the_same_draws(which):
    from gm3d_amd import data_transforms as T
    B, N = 5, 1000
    chain = chain_a(T) if which == "chainA" else every_op(T)
    prog = T.Program(chain)
    pc = clouds_for(B, N, 3)
    gen = torch.Generator(device="cuda").manual_seed(5)
    got = T.Compose(chain)(pc.cuda(), generator=gen)
    gen.manual_seed(5)                                                     # the same three calls again
    cu = torch.rand(B, prog.D, device="cuda", generator=gen).view(-1)
    pu = torch.rand(B, N, device="cuda", generator=gen)
    pz = torch.randn(B, N, 3, device="cuda", generator=gen)
    want = T.augment_torch(pc.clone(), prog, cu.cpu(), pu.cpu(), pz.cpu())
    assert not torch.equal(want, pc)
    check(got.cpu().numpy(), want.numpy(), ["rotate"] if which == "every_op" else ["chainA"], "live " + which)
    again = T.Compose(chain)(pc.cuda(), generator=gen)                     # the generator moved on: other draws
    assert not torch.equal(again, got)


# ------------------------------------------------------------------------------------------------ (d) captured
def test_captured_chain_replays_with_fresh_draws():
    """chain A captured on its own generator (never the default one, whose state other captured graphs share): every replay draws
    anew, and equals the restatement on the draws the generator's state at that replay gives"""
    from gm3d_amd import data_transforms as T
    B, N = 4, 1000
    chain = T.Compose(chain_a(T))
    prog = T.Program(chain.transforms)
    pc = clouds_for(B, N, 8)
    static = pc.cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    chain(static.clone(), generator=gen)                                   # eager once: code objects loaded before the capture
    torch.cuda.synchronize()
    default_before = torch.cuda.get_rng_state()
    graph = torch.cuda.CUDAGraph()
    graph.register_generator_state(gen)
    with torch.cuda.graph(graph):
        out = chain(static.clone(), generator=gen)
    outs = []
    for _ in range(2):
        twin = torch.Generator(device="cuda")
        twin.set_state(gen.get_state())                                    # what this replay will draw from
        graph.replay()
        torch.cuda.synchronize()
        cu = torch.rand(B, prog.D, device="cuda", generator=twin).view(-1)
        pu = torch.rand(B, N, device="cuda", generator=twin)
        pz = torch.randn(B, N, 3, device="cuda", generator=twin)
        want = T.augment_torch(pc.clone(), prog, cu.cpu(), pu.cpu(), pz.cpu())
        check(out.cpu().numpy(), want.numpy(), ["chainA"], "replay %d" % len(outs))
        outs.append(out.clone())
    assert not torch.equal(outs[0], outs[1])
    assert torch.equal(static.cpu(), pc)                                   # the captured clone is what was augmented
    assert torch.equal(torch.cuda.get_rng_state(), default_before)         # the default generator was left alone


# ------------------------------------------------------------------------------------------------ (e) the older kernel
def test_compose_of_scale_and_translate_equals_train_transforms():
    from gm3d_amd import data_transforms as T
    from gm3d_amd import engine_pretrain as E
    pc = clouds_for(5, 1000, 13).cuda()
    gen = torch.Generator(device="cuda").manual_seed(21)
    old = E.train_transforms(pc.clone(), generator=gen)
    gen.manual_seed(21)
    new = T.Compose([T.PointcloudScaleAndTranslate()])(pc.clone(), generator=gen)
    assert not torch.equal(old, pc)
    assert torch.equal(new, old)


# ------------------------------------------------------------------------------------------------ (f) inside the captured step
def test_chain_a_inside_the_captured_point_mae_step(monkeypatch):
    """chain A as engine_pretrain_point_mae.train_transforms (fed static draws, so that eager and replay see the same ones): the step
    captures, the loss is finite, and replay equals eager bit for bit from identical state -- loss, parameters, both moments"""
    from gm3d_amd import data_transforms as T
    from gm3d_amd import engine_pretrain_point_mae as EP
    from tests import clouds
    from tests.test_gpu_point_mae_pretrain import _args, _model
    B, G, N = 4, 64, 1024
    chain = T.Compose(chain_a(T))
    static_draws = [tuple(v.cuda() for v in d) if isinstance(d, tuple) else d.cuda() for d in injected(T, chain.transforms, B, N, 77)]
    seen = []

    def transforms(pc, draws=None, generator=None):
        seen.append(pc.shape)
        return chain(pc, draws=static_draws)
    monkeypatch.setattr(EP, "train_transforms", transforms)
    m = _model("rand", drop_path=0.0, num_group=G)
    opt = EP.build_optimizer(m)
    args = _args()
    x = [clouds.gaussian(B, N, seed=900 + i).cuda() for i in range(2)]
    gen = torch.Generator().manual_seed(23)
    noise = [torch.rand(B, G, generator=gen).cuda() for _ in range(2)]
    g = EP.GraphedPointMAEStep(m, opt, x[0], args, warmup_iters=2, augment=True, inject_mask_noise=True)
    calls = len(seen)                                                      # the warm-up steps and the capture
    assert calls >= 1
    state = ({k: v.clone() for k, v in m.state_dict().items()}, opt.M.clone(), opt.V.clone(), opt.step_dev.clone())

    def restore():
        with torch.no_grad():
            m.load_state_dict(state[0])
            opt.M.copy_(state[1]); opt.V.copy_(state[2]); opt.step_dev.copy_(state[3])
            opt.sync_shadows()

    restore()
    want = []
    for i in range(2):
        o = EP.pretrain_step(m, opt, x[i].clone(), args, mask_noise=noise[i], augment=True, micro_step=i)
        want.append((o["loss"].clone(), opt.P.clone(), opt.M.clone(), opt.V.clone()))
    restore()
    for i in range(2):
        o = g(x[i], mask_noise=noise[i])
        got = (o["loss"], opt.P, opt.M, opt.V)
        assert bool(torch.isfinite(got[0]))
        assert all(torch.equal(a, b) for a, b in zip(got, want[i])), (i, float(got[0]), float(want[i][0]))
        assert torch.equal(g.static_in, chain(x[i].clone(), draws=static_draws)) and not torch.equal(g.static_in, x[i])
    assert len(seen) == calls + 2                                          # the two eager steps; the replays ran no Python

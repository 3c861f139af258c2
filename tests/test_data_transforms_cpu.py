"""CPU: gm3d_amd/data_transforms.py -- the torch restatement of gm3d_augment against the reference's own transforms
(tests/golden/data_transforms.npz, made by tests/golden/make_golden_data_transforms.py), the program encoding, the launch split and
the entry point's argument checks.

Bars (derived, not tuned).  Every op except the rotation is one or two separately rounded float32 operations on operands identical
to the reference's, and the flip's maximum is exact: torch.equal.  The rotation: c and s are each within one float32 ulp of the
reference's after the double -> float32 cast, and the reference's matmul forms two products and one sum, fused or not; that is at
most 3.5 * sqrt(2) ulp of the cloud's largest |coordinate|, rounded up to 8 * 2^-24 = 2^-21."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "data_transforms.npz")
SIZES = (1, 33, 1000)
OPS = ("rotate", "scale", "translate", "scale_translate", "jitter", "dropout", "flip")
CHAINS = {"chainA": ("scale", "translate", "jitter", "dropout", "flip"),
          "chainB": ("flip", "dropout", "scale_translate", "jitter", "rotate")}
ROT_BAR = 2.0 ** -21
JITTER = dict(std=0.01, clip=0.02)           # the fixture's jitter (jitter_std_clip): a clip that bites; every other op has the defaults


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLD)


def make(name):
    from gm3d_amd import data_transforms as T
    return {"rotate": T.PointcloudRotate, "scale": T.PointcloudScale, "translate": T.PointcloudTranslate,
            "scale_translate": T.PointcloudScaleAndTranslate, "jitter": T.PointcloudJitter,
            "dropout": T.PointcloudRandomInputDropout, "flip": T.RandomHorizontalFlip}[name](**(JITTER if name == "jitter" else {}))


def stored_draws(fx, prefix, name):
    """the fixture's draws of one op -> its `draws=` entry"""
    g = lambda k: torch.from_numpy(fx["%s/%s/%s" % (prefix, name, k)])
    return {"rotate": lambda: g("u"), "scale": lambda: g("scale"), "translate": lambda: g("shift"),
            "scale_translate": lambda: (g("scale"), g("shift")), "jitter": lambda: g("noise"),
            "dropout": lambda: (g("ratio"), g("point_u")), "flip": lambda: g("u")}[name]()


def case(fx, N, what):
    """-> (names, input (B,N,3) tensor, draws list, the reference's output) for an op name or a chain name"""
    names = CHAINS.get(what, (what,))
    prefix = "n%d/%s" % (N, what) if what in CHAINS else "n%d" % N
    return names, torch.from_numpy(fx["n%d/pc" % N].copy()), [stored_draws(fx, prefix, n) for n in names], fx["n%d/%s/out" % (N, what)]


def check(got, want, names, label=""):
    """got / want (B,N,3) arrays under the bars of the module docstring; prints the figure it asserts on"""
    got, want = np.asarray(got), np.asarray(want)
    if "rotate" not in names:
        print("%s %s: %d of %d elements differ" % (label, "+".join(names), int((got != want).sum()), got.size))
        assert np.array_equal(got, want)
        return
    B = want.shape[0]
    err = np.abs(got.astype(np.float64) - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)
    print("%s %s: error / largest coordinate per cloud %s, bar %.3e" % (label, "+".join(names), err, ROT_BAR))
    assert (err <= ROT_BAR).all()


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("what", OPS + tuple(CHAINS))
def test_fallback_equals_reference(fx, N, what):
    from gm3d_amd import data_transforms as T
    names, pc, draws, want = case(fx, N, what)
    t = T.Compose([make(n) for n in names])
    out = t(pc, draws=draws)
    assert out is pc                                           # in place, and returned
    check(pc.numpy(), want, names)
    if what in OPS and what != "scale_translate":              # the transform called on its own, like the reference's
        x = torch.from_numpy(fx["n%d/pc" % N].copy())
        assert make(what)(x, draws=draws[0]) is x
        assert torch.equal(x, pc)


def test_fixture_is_not_vacuous(fx):
    """every op moved the clouds, the dropout dropped some points and kept others, the flip flipped and the gate / coin held too"""
    for what in OPS + tuple(CHAINS):
        assert not np.array_equal(fx["n1000/%s/out" % what], fx["n1000/pc"]), what
    drop = fx["n1000/dropout/point_u"] <= fx["n1000/dropout/ratio"][:, None]
    assert drop.any() and not drop.all()
    u = np.concatenate([fx["n%d/flip/u" % N] for N in SIZES] + [fx["n%d/%s/flip/u" % (N, c)] for N in SIZES for c in CHAINS])
    assert (u[:, 1] < 0.5).any() and (u[:, 1] >= 0.5).any() and (u[:, 2] < 0.5).any() and (u[:, 2] >= 0.5).any()
    noise = fx["n1000/jitter/noise"]
    assert list(fx["jitter_std_clip"]) == [JITTER["std"], JITTER["clip"]]
    assert (np.abs(noise) > JITTER["clip"]).any() and (np.abs(noise) < JITTER["clip"]).any()      # the clamp bites


def test_fallback_handles_strided_and_other_dtypes(fx):
    from gm3d_amd import data_transforms as T
    names, pc, draws, want = case(fx, 33, "chainA")
    t = T.Compose([make(n) for n in names])
    wide = torch.zeros(4, 33, 5)
    view = wide[:, :, 1:4]
    view.copy_(pc)
    assert t(view, draws=draws) is view
    check(view.numpy(), want, names)
    assert bool((wide[:, :, 0] == 0).all()) and bool((wide[:, :, 4] == 0).all())
    dbl = pc.double()
    t(dbl, draws=draws)
    check(dbl.float().numpy(), want, names)                    # computed in float32, stored as float64: exact


def test_live_draws_need_at_most_three_calls(monkeypatch):
    """one torch.rand(B, D), torch.rand(B, N) only with a dropout, torch.randn(B, N, 3) only with a jitter -- on the given generator"""
    from gm3d_amd import data_transforms as T
    calls = []
    rand, randn = torch.rand, torch.randn
    monkeypatch.setattr(torch, "rand", lambda *a, **k: calls.append(("rand", a, k.get("generator"))) or rand(*a, **k))
    monkeypatch.setattr(torch, "randn", lambda *a, **k: calls.append(("randn", a, k.get("generator"))) or randn(*a, **k))
    g = torch.Generator().manual_seed(3)
    pc = torch.ones(2, 5, 3)
    T.Compose([make(n) for n in CHAINS["chainA"]])(pc, generator=g)
    assert [(c[0], c[1]) for c in calls] == [("rand", (2, 10)), ("rand", (2, 5)), ("randn", (2, 5, 3))]
    assert all(c[2] is g for c in calls)
    del calls[:]
    T.Compose([T.PointcloudRotate(), T.PointcloudScale()])(pc, generator=g)
    assert [(c[0], c[1]) for c in calls] == [("rand", (2, 4))]
    del calls[:]
    T.PointcloudJitter()(pc, generator=g)
    assert [(c[0], c[1]) for c in calls] == [("randn", (2, 5, 3))]


def test_live_draws_equal_injected_draws():
    """the live path's quantities are the documented maps of its uniforms: re-seed, draw the same tensors, inject the finals"""
    from gm3d_amd import data_transforms as T
    B, N = 3, 17
    chain = [T.PointcloudScale(0.5, 2.0), T.PointcloudTranslate(0.3), T.PointcloudJitter(0.02, 0.03), T.PointcloudRandomInputDropout(0.5),
             T.RandomHorizontalFlip("y"), T.PointcloudRotate(), T.PointcloudScaleAndTranslate()]
    pc = torch.rand(B, N, 3, generator=torch.Generator().manual_seed(1)) - 0.5
    live = T.Compose(chain)(pc.clone(), generator=torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    cu = torch.rand(B, 17, generator=g).view(-1)
    point_u, point_z = torch.rand(B, N, generator=g), torch.randn(B, N, 3, generator=g)
    grp = lambda col, cnt: T._group(cu, B, col, cnt)
    draws = [grp(0, 3) * 1.5 + 0.5, (grp(3, 3) * 2 - 1) * T._f32(0.3), point_z * T._f32(0.02), (grp(6, 1)[:, 0] * 0.5, point_u), grp(7, 3),
             grp(10, 1)[:, 0], (grp(11, 3) * T._f32(1.5 - 2. / 3.) + T._f32(2. / 3.), (grp(14, 3) * 2 - 1) * T._f32(0.2))]
    assert torch.equal(T.Compose(chain)(pc.clone(), draws=draws), live)
    assert not torch.equal(live, pc)
    half = T.Compose(chain)(pc.clone(), draws=[None, draws[1], None, None, draws[4], None, None], generator=torch.Generator().manual_seed(9))
    assert torch.equal(half, live)                             # None entries are drawn live, from the same columns


def test_flip_axes_follow_the_upright_axis():
    from gm3d_amd import data_transforms as T
    pc = torch.tensor([[[1.0, 2.0, 3.0], [4.0, 6.0, 9.0]]])
    u = torch.tensor([[0.1, 0.2, 0.9]])                        # gate passes, the lower axis flips, the higher does not
    for up, ax in (("z", 0), ("y", 0), ("x", 1)):
        out = T.RandomHorizontalFlip(up)(pc.clone(), draws=u)
        want = pc.clone()
        want[0, :, ax] = pc[0, :, ax].max() - pc[0, :, ax]
        assert torch.equal(out, want), up
    above = float(np.nextafter(np.float32(0.95), np.float32(1)))           # float32(0.95) itself is below the double 0.95
    assert torch.equal(T.RandomHorizontalFlip()(pc.clone(), draws=torch.tensor([[above, 0.0, 0.0]])), pc)
    assert not torch.equal(T.RandomHorizontalFlip()(pc.clone(), draws=torch.tensor([[0.95, 0.0, 0.0]])), pc)
    out = T.RandomHorizontalFlip()(pc.clone(), draws=torch.tensor([[0.0, 0.5, float(np.nextafter(np.float32(0.5), np.float32(0)))]]))
    assert torch.equal(out[..., 0], pc[..., 0]) and torch.equal(out[0, :, 1], torch.tensor([4.0, 0.0]))       # 0.5 < 0.5 is false
    assert T.RandomHorizontalFlip().horz_axes == {0, 1} and T.RandomHorizontalFlip().D == 3


def test_is_temporal_is_refused():
    from gm3d_amd import data_transforms as T
    with pytest.raises(NotImplementedError):
        T.RandomHorizontalFlip(is_temporal=True)


def test_constructor_defaults_are_the_references():
    from gm3d_amd import data_transforms as T
    from gm3d_amd import engine_pretrain as E
    assert T.PointcloudScaleAndTranslate is E.PointcloudScaleAndTranslate
    assert (T.PointcloudJitter().std, T.PointcloudJitter().clip) == (0.01, 0.05)
    assert (T.PointcloudScale().scale_low, T.PointcloudScale().scale_high) == (2. / 3., 3. / 2.)
    assert T.PointcloudTranslate().translate_range == 0.2
    assert T.PointcloudRandomInputDropout().max_dropout_ratio == 0.5
    assert T.RandomHorizontalFlip().upright_axis == 2
    with pytest.raises(AssertionError):
        T.PointcloudRandomInputDropout(1.0)
    with pytest.raises(TypeError):
        T.Compose([lambda pc: pc])


def test_program_encoding_and_column_offsets():
    from gm3d_amd import data_transforms as T
    p = T.Program([make(n) for n in CHAINS["chainA"]])
    assert p.codes == [T.SCALE, T.TRANSLATE, T.JITTER, T.DROPOUT, T.FLIP]
    assert p.cols == [0, 3, 6, 6, 7] and p.D == 10
    f = T._f32
    assert p.params == [(f(2. / 3.), f(1.5 - 2. / 3.), 0.0), (f(0.2), 0.0, 0.0), (f(0.01), f(0.02), 0.0), (0.5, 0.0, 0.0), (2.0, 0.0, 0.0)]
    p = T.Program([make(n) for n in CHAINS["chainB"]], final=[True] * 5)
    assert p.codes == [T.FLIP, T.DROPOUT | T.FINAL, T.SCALE_TRANSLATE | T.FINAL, T.JITTER | T.FINAL, T.ROTATE]
    assert p.cols == [0, 3, 4, 10, 10] and p.D == 11
    assert p.params[2] == (f(2. / 3.), f(1.5 - 2. / 3.), f(0.2))
    assert T.Program([T.RandomHorizontalFlip("x")]).params == [(0.0, 0.0, 0.0)]
    with pytest.raises(ValueError):
        T.Program([T.PointcloudRotate()] * 9)
    with pytest.raises(ValueError):
        T.Program([T.PointcloudJitter(), T.PointcloudJitter()])
    # the codes are the header's
    txt = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "gm3d.h")).read()
    for name in ("ROTATE", "SCALE", "TRANSLATE", "SCALE_TRANSLATE", "JITTER", "DROPOUT", "FLIP"):
        assert "GM3D_AUG_%s = %d," % (name, getattr(T, name)) in txt
    assert "GM3D_AUG_FINAL = 0x%x," % T.FINAL in txt and "GM3D_AUG_MAX_OPS = %d\n" % T.MAX_OPS in txt


def test_long_chains_are_split_into_consecutive_launches():
    from gm3d_amd import data_transforms as T
    rot, jit, drop = T.PointcloudRotate(), T.PointcloudJitter(), T.PointcloudRandomInputDropout()
    assert T.split([rot] * 8) == [(0, 8)]
    assert T.split([rot] * 9) == [(0, 8), (8, 9)]
    assert T.split([rot] * 17) == [(0, 8), (8, 16), (16, 17)]
    assert T.split([jit, rot, jit, drop, drop]) == [(0, 2), (2, 4), (4, 5)]
    assert T.split([]) == []
    # 11 ops: the same result as the ops one after the other, on the same injected draws
    B, N = 2, 9
    g = torch.Generator().manual_seed(4)
    chain, draws = [], []
    for i in range(11):
        if i % 3 == 0:
            chain.append(T.PointcloudScale()); draws.append(torch.rand(B, 3, generator=g) + 0.5)
        elif i % 3 == 1:
            chain.append(T.PointcloudJitter()); draws.append(torch.randn(B, N, 3, generator=g) * 0.03)
        else:
            chain.append(T.RandomHorizontalFlip()); draws.append(torch.rand(B, 3, generator=g))
    pc = torch.rand(B, N, 3, generator=g)
    t = T.Compose(chain)
    assert t.launches == [(0, 4), (4, 7), (7, 10), (10, 11)]          # a second jitter opens a new launch
    want = pc.clone()
    for op, d in zip(chain, draws):
        op(want, draws=d)
    assert torch.equal(t(pc.clone(), draws=draws), want) and not torch.equal(want, pc)


def test_argument_errors_are_detected_before_any_launch():
    """gm3d_augment on the host: safe without a GPU (no pointer is dereferenced on the device side before the checks pass)"""
    from gm3d_amd import data_transforms as T
    from gm3d_amd._capi import GM3D_EINVAL, GM3D_OK, lib
    one = ctypes.c_void_p(16)

    def call(codes, pc=one, B=0, N=4, nops=None, params=True, cloud_u=one, point_u=one, point_z=one, p0=2.0):
        ops = (ctypes.c_int * max(len(codes), 1))(*codes)
        par = (ctypes.c_float * (3 * max(len(codes), 1)))(*([p0, 0.0, 0.0] * len(codes)))
        return lib.gm3d_augment(pc, B, N, len(codes) if nops is None else nops, ops if codes else None, par if params else None,
                                cloud_u, point_u, point_z, None)

    every = [T.ROTATE, T.SCALE, T.TRANSLATE, T.SCALE_TRANSLATE, T.JITTER, T.DROPOUT, T.FLIP, T.SCALE | T.FINAL]
    assert call(every) == GM3D_OK                              # B = 0: success, nothing launched
    assert call(every, pc=None) == GM3D_EINVAL
    assert call(every, N=0) == GM3D_EINVAL
    assert call(every, B=-1) == GM3D_EINVAL
    assert call([]) == GM3D_EINVAL and call(every, nops=0) == GM3D_EINVAL
    assert call(every + [T.ROTATE]) == GM3D_EINVAL             # nine ops
    assert call(every, params=False) == GM3D_EINVAL
    assert call([0]) == GM3D_EINVAL and call([8]) == GM3D_EINVAL and call([T.ROTATE | 0x200]) == GM3D_EINVAL
    assert call([T.FLIP], p0=3.0) == GM3D_EINVAL and call([T.FLIP], p0=0.5) == GM3D_EINVAL
    assert call([T.ROTATE], cloud_u=None) == GM3D_EINVAL
    assert call([T.JITTER], cloud_u=None) == GM3D_OK           # D = 0: no cloud_u needed
    assert call([T.JITTER], point_z=None) == GM3D_EINVAL
    assert call([T.DROPOUT], point_u=None) == GM3D_EINVAL
    assert call([T.ROTATE], point_u=None, point_z=None) == GM3D_OK
    assert call([T.JITTER, T.JITTER]) == GM3D_EINVAL and call([T.DROPOUT, T.ROTATE, T.DROPOUT]) == GM3D_EINVAL
    # bad arguments are refused for a real batch as well, before anything is launched
    assert call(every, B=4, N=0) == GM3D_EINVAL and call([9], B=4) == GM3D_EINVAL

"""-m gpu: the product's bf16 step (the arithmetic bench.py times: own MFMA GEMMs, bf16 MFMA attention, bf16 LayerNorm / GELU
outputs) against the REFERENCE's fp32 fixtures, per tensor.

Yardstick: tests/golden/pretrain_bf16.npz (tests/golden/make_golden_bf16.py) holds, next to the fp32 gradient norm of every live
parameter and an element-wise sample of one gradient per GEMM family (every 4th row and column: all 64 x 64 blocks covered), the
reference's OWN error when it runs the same step under CPU
bf16 autocast ("ac_err").  A tensor's bar is MULT x that error: a bar scaled to how sensitive that tensor is to 8-bit mantissas
(the losses move ~5e-4, the first-layer gradients ~8e-2).  On top of that, localized errors -- one wrong tile, one wrong cloud
-- are caught by the tile check of tests/parity.py, which whole-tensor errors at these bars cannot see.

The step runs as step_forward_backward runs it: weight_cache pinned and refreshed, teacher eval forward and student train forward
under torch.autocast("cuda", bfloat16), backward through engine_pretrain.backward_and_collect (the async weight-gradient
stream).  The inputs, mask_e200 and DropPath keep-masks are the fp32 fixture's, replayed (FeedDropPath)."""
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as R
from tests.parity import Ledger
from tests.test_gpu_model import FeedDropPath

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

MULT = 3.0            # bar = MULT x the reference's own bf16-autocast error.  Worst measured/bar on the MI355X: b2_uniform 0.43
                      # (chamfer_mean), b4_gaussian 0.39 (blocks.0.attn.proj.weight gradient sample); the product's
                      # bf16 step sits at about the reference's own autocast error, tensor by tensor
NOISE_REL = 1e-5      # a gradient whose fp32 norm is below NOISE_REL x the norm of all gradients is analytically zero (a bias
NOISE_FLOOR = 1e-4    # feeding a BatchNorm): only rounding noise is left; its bar is NOISE_FLOOR x the norm of all gradients
COS_MIN = 0.999       # cosine similarity, for tensors whose reference autocast error is below COS_WHERE
COS_WHERE = 1e-2
TILE_FLOOR = 1e-3     # tile check: blocks whose max |error| is below TILE_FLOOR x max |reference| are not judged


@pytest.fixture(scope="module")
def M():
    from gm3d_amd import models_mae_learn_loss as M
    return M


@pytest.fixture(scope="module")
def model(M):
    """A model of this module's own: pinning the weight cache changes the module fixture of test_gpu_model.py."""
    torch.manual_seed(0)
    m = M.mae_vit_base_patch16_dec512d8b(norm_pix_loss=False)
    R.det_fill_(m, seed=0)
    return m.cuda()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "pretrain_bf16.npz"))


def _step(M, model, fx, monkeypatch):
    from gm3d_amd import engine_pretrain as E
    from gm3d_amd.fused import weight_cache
    samples = torch.from_numpy(fx["samples"]).cuda()
    B = samples.shape[0]
    weight_cache.pin(model)
    weight_cache.refresh()
    out = {}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        model.eval()
        with torch.no_grad():
            vis = torch.zeros(B, 64, dtype=torch.bool, device="cuda")
            t = model(samples, mask=vis)
            out["teacher_noaug"] = model(samples, mask=vis, noaug=True)
        for k in ("features", "pix_pred", "loss_pred"):
            out["teacher_" + k] = t[k]
        model.train()
        mask = torch.from_numpy(fx["mask_e200"]).bool().cuda()
        feed = FeedDropPath(fx["droppath_masks"])
        monkeypatch.setattr(M, "drop_path", feed)
        monkeypatch.setattr(M, "drop_path_scale", feed.scale)
        s = model(samples, mask=mask)
        assert feed.masks == []
        Mn = int(fx["mask_num"])
        assert s["mask_num"] == Mn
        lo = model.forward_loss(s["pix_pred"][:, -Mn:], s["neighborhood"], s["mask"])
        ll = model.forward_learning_loss(s["loss_pred"][:, -Mn:], mask, lo["matrix"].detach(), relative=True)
        loss = lo["Chamfer_mean"] if lo.get("MSE_zero") else 13.889 * lo["MSE_mean"] + lo["Chamfer_mean"]
    assert float(lo["MSE_mean"]) == 0.0
    E.backward_and_collect((loss, ll), model, None, None)
    out.update({"student_features": s["features"], "student_pix_pred": s["pix_pred"], "student_loss_pred": s["loss_pred"],
                "matrix": lo["matrix"], "chamfer_mean": lo["Chamfer_mean"], "loss_learn": ll})
    torch.cuda.synchronize()
    return out


def grad_bars(gold, prefix, names, norms):
    """-> {name: absolute L2 bar} for every live parameter: MULT x the reference's autocast error, or the noise floor."""
    total = float(np.sqrt((norms ** 2).sum()))
    abs_err = gold[prefix + "ac_abs_grad"]
    return {n: (max(MULT * float(a), NOISE_FLOOR * total) if float(g) <= NOISE_REL * total else MULT * float(a))
            for n, g, a in zip(names, norms, abs_err)}


@pytest.mark.parametrize("case", ["b2_uniform", "b4_gaussian"])
def test_bf16_step_against_reference_fp32(M, model, gold, case, monkeypatch):
    """The fused transformer stacks only (FUSED_STACK, the bench path).  The per-op modules (FUSED_STACK = False, the fp32
    cross-check path of test_gpu_model.py) have no bf16 training route: run this way under autocast, 140 of the 251 live
    parameters -- the transformer blocks' -- receive no gradient at all, so there is nothing to hold to these bars."""
    monkeypatch.setattr(M, "FUSED_STACK", True)
    fx = np.load(os.path.join(GOLD, "pretrain_%s.npz" % case))
    saved = {k: v.clone() for k, v in model.state_dict().items()}
    try:
        out = _step(M, model, fx, monkeypatch)
        _judge(model, gold, fx, case, out)
    finally:
        model.load_state_dict(saved)
        model.zero_grad()


def _judge(model, gold, fx, case, out):
    pre = case + "/"
    led = Ledger("%s bf16 vs reference fp32 (bar = %.0f x reference autocast error)" % (case, MULT))
    # activations and losses (worst measured/bar: chamfer_mean 0.43 at b2, all others below 0.33)
    for k in ("teacher_features", "teacher_noaug", "teacher_pix_pred", "teacher_loss_pred", "student_features", "student_pix_pred",
              "student_loss_pred", "matrix", "chamfer_mean", "loss_learn"):
        ref = fx[k]
        ac = float(gold[pre + "ac_err::" + k])
        led.rel(k, out[k], ref, MULT * ac)
        if ref.size > 1:
            led.cos(k, out[k], ref, COS_MIN)
            led.tiles(k, out[k], ref, "act", floor=TILE_FLOOR * float(np.abs(ref).max()))
    # BatchNorm running statistics after the step (the reference autocast error is 0 for the BNs the step does not touch)
    sd = model.state_dict()
    for k in fx.files:
        if k.startswith("bn_after::"):
            led.rel(k, sd[k[10:]], fx[k], max(MULT * float(gold[pre + "ac_err::" + k]), 1e-6))

    named = dict(model.named_parameters())
    names = [str(n) for n in gold["param_names"]]
    norms = gold[pre + "gradnorm_all"]
    bars = grad_bars(gold, pre, names, norms)
    assert sorted(names) == sorted(k for k, p in named.items() if p.grad is not None), "live-parameter set"
    # every live gradient's norm: | |g| - |g_ref| | <= |g - g_ref| <= its bar
    for n, g_ref in zip(names, norms):
        led.add("gradnorm %s" % n, abs(float(named[n].grad.double().norm()) - float(g_ref)), bars[n])
    # the sampled gradients (one tensor per GEMM family: every SAMPLE-th row and column, each 64 x 64 block represented) and the
    # fp32 fixture's own (small tensors whole, big ones their first 24 rows): L2 error, cosine, tiles
    stride = int(gold["sample_stride"])
    sampled = [k[len(pre) + len("grad_sample::"):] for k in gold.files if k.startswith(pre + "grad_sample::")]
    for n in sampled:
        ref = gold[pre + "grad_sample::" + n].astype(np.float64) * float(gold[pre + "grad_scale::" + n])
        g = named[n].grad.reshape(named[n].shape[0], -1)[::stride, ::stride]
        _grad_checks(led, "grad_sample " + n, g, ref, MULT * float(gold[pre + "ac_abs_sample::" + n]),
                     float(gold[pre + "ac_err_grad"][names.index(n)]), stride)
    for key in fx.files:
        if key.startswith("grad::") and key[6:] not in sampled:
            n = key[6:]
            g = named[n].grad
            ref = fx[key]
            bar = bars[n]
            if g.numel() > 65536:       # the fixture keeps the first 24 rows: their share of the bar follows their share of the norm
                g = g[: ref.shape[0]]
                bar *= float(np.linalg.norm(ref)) / float(fx["gradnorm::" + n])
            _grad_checks(led, "grad " + n, g, ref, bar, float(gold[pre + "ac_err_grad"][names.index(n)]))
    print(led.report(12))
    led.assert_ok()


def _grad_checks(led, label, g, ref, bar_abs, ac, stride=1):
    g = g.detach().double().cpu().reshape(ref.shape)
    ref_t = torch.from_numpy(np.asarray(ref, dtype=np.float64))
    led.add(label + " L2 err", float((g - ref_t).norm()), bar_abs)
    if np.isfinite(ac) and ac <= COS_WHERE:
        led.cos(label, g, ref_t, COS_MIN)
    if ref_t.dim() >= 2:
        led.tiles(label, g, ref_t, "weight", floor=TILE_FLOOR * float(ref_t.abs().max()), stride=stride)

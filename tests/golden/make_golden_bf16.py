"""Generates tests/golden/pretrain_bf16.npz: the reference's own fp32 gradients of EVERY live parameter and the reference's own
bf16-autocast error, the yardsticks of the bf16 parity tests (tests/test_gpu_bf16_parity.py, tests/test_gpu_b128.py).

The reference model file is imported in place exactly as tests/golden/make_golden.py does it (same stand-ins for the absent
packages, same det_fill_ weights).  For each existing fixture case (b2_uniform, b4_gaussian) the fp32 run replays that fixture's
inputs, mask_e200 and DropPath keep-masks, and is first checked to reproduce every stored key of pretrain_<case>.npz bit for bit.
The same step is then run under torch.autocast("cpu", bfloat16) with the SAME mask and keep-masks (re-drawing them changes which
samples are dropped -- a 29 % feature difference that is not arithmetic); FPS/KNN/Chamfer are the oracle's fp32 C code either way
and the reference itself casts the Chamfer operands to fp32 (models_mae_learn_loss.py:400-401).

Keys ("<case>/" prefix; the per-parameter arrays are indexed like `param_names`, the manifest's live_parameters):
  param_names                 the 251 live parameters, in state_dict_manifest.json order
  sample_stride               SAMPLE (below)
  <case>/gradnorm_all         fp32 gradient L2 norm of every live parameter (float64 [251])
  <case>/ac_err_grad          rel-L2 error ||autocast - fp32|| / ||fp32|| of every live gradient (nan where the fp32 gradient
                              is exactly zero: biases feeding a BatchNorm or a mean-invariant loss)
  <case>/ac_abs_grad          the same error, absolute (||autocast - fp32||)
  <case>/ac_err::<key>        the same rel-L2 error of an activation (teacher_*, student_*, matrix, chamfer_mean, loss_learn)
                              or of a BatchNorm running statistic after the step (bn_after::<name>)
  <case>/grad_sample::<name>  fp32 gradient of one tensor per GEMM family, element by element on a regular sub-grid: viewed as
                              2-D [out, in], every SAMPLE-th row and column, i.e. a (64/SAMPLE)^2 sample of each 64 x 64 block,
                              so that every block of the tensor is covered (tests/parity.py tile check, stride=SAMPLE).  Divided
                              by <case>/grad_scale::<name> (the sample's max |element|) and stored as float16 (relative
                              rounding <= 2^-11).  The whole tensors would make a multi-megabyte fixture.
  <case>/ac_abs_sample::<name> ||autocast - fp32|| of the reference on that same sample (the bar of the sample's L2 error)
and, for tests/test_gpu_b128.py, "b128/" arrays of the same kind (gradnorm_all, ac_err_grad, ac_abs_grad, ac_err::<key>, grad_norm):
B=128 clouds.uniform(128, 1024, B128_CLOUD_SEED), mask noise torch.rand(128, 64) from B128_NOISE_SEED, epoch 0 (mask = the noise
ranking, no teacher guidance), DropPath off.

Deterministic: torch runs with THREADS intra-op threads (CPU reduction order depends on the thread count); two runs write
byte-identical files.  Usage:  python tests/golden/make_golden_bf16.py   (writes next to this file; well under a minute)
"""
import io
import os
import sys
import zipfile
from contextlib import nullcontext

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import model_ref as R  # noqa: E402
from tests import clouds  # noqa: E402
from tests.golden.make_golden import REF, install_absent_packages  # noqa: E402

THREADS = 8
CASES = ("b2_uniform", "b4_gaussian")
SAMPLE = 4
# one tensor per GEMM family: encoder block (qkv / proj / fc1 / fc2), the encoder's second conv, the loss head's first conv,
# one decoder block weight
GRAD_SAMPLED = ("blocks.blocks.0.attn.qkv.weight", "blocks.blocks.0.attn.proj.weight", "blocks.blocks.0.mlp.fc1.weight",
             "blocks.blocks.0.mlp.fc2.weight", "encoder.second_conv.0.weight", "increase_dim_2.0.weight",
             "MAE_decoder.blocks.0.attn.proj.weight")
ACT_KEYS = ("teacher_features", "teacher_noaug", "teacher_pix_pred", "teacher_loss_pred", "student_features", "student_pix_pred",
            "student_loss_pred", "matrix", "chamfer_mean", "loss_learn")
B128, B128_CLOUD_SEED, B128_NOISE_SEED = 128, 150, 0


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def epoch0_mask(noise, mask_ratio=0.6):
    """generate_mask at epoch 0 (no guided tokens) with the random ranking given by `noise`: the len_keep lowest stay visible."""
    B, L = noise.shape
    len_keep = int(L * (1 - mask_ratio))
    mask = torch.ones(B, L)
    mask.scatter_(1, torch.argsort(noise, dim=1)[:, :len_keep], 0.0)
    return mask


def bn_state(ref):
    return {k: v.clone() for k, v in ref.state_dict().items() if "running" in k or k.endswith("num_batches_tracked")}


def restore(ref, snap):
    with torch.no_grad():
        sd = ref.state_dict()
        for k, v in snap.items():
            sd[k].copy_(v)


def run_step(ref, samples, mask, droppath, amp, teacher_noaug=True):
    """Teacher eval forward (all visible) -> student train forward with `mask` and the given DropPath keep-masks -> the
    reference's objective -> backward.  Returns float64 numpy activations and fp32 gradients."""
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if amp else nullcontext()
    B = samples.shape[0]
    out = {}
    ref.eval()
    vis = torch.zeros(B, 64, dtype=torch.bool)
    with ctx, torch.no_grad():
        t = ref(samples.clone(), mask=vis)
        if teacher_noaug:
            out["teacher_noaug"] = ref(samples.clone(), mask=vis, noaug=True)
    for k in ("features", "pix_pred", "loss_pred"):
        out["teacher_" + k] = t[k]
    out["neighborhood"] = t["neighborhood"]
    ref.train()
    R._droppath_feed = [torch.from_numpy(m) for m in droppath] if droppath is not None else None
    try:
        with ctx:
            s = ref(samples.clone(), mask=mask)
            M = s["mask_num"]
            lo = ref.forward_loss(s["pix_pred"][:, -M:], s["neighborhood"], s["mask"])
            ll = ref.forward_learning_loss(s["loss_pred"][:, -M:], mask, lo["matrix"].detach(), relative=True)
            total = 13.889 * lo["MSE_mean"] + 1.0 * lo["Chamfer_mean"] + ll   # engine_pretrain.py:153,190
        assert R._droppath_feed is None or R._droppath_feed == [], "DropPath keep-masks left over"
    finally:
        R._droppath_feed = None
    ref.zero_grad()
    total.backward()
    out.update({"student_features": s["features"], "student_pix_pred": s["pix_pred"], "student_loss_pred": s["loss_pred"],
                "matrix": lo["matrix"], "chamfer_mean": lo["Chamfer_mean"], "loss_learn": ll})
    out = {k: v.detach().double().numpy() for k, v in out.items()}
    grads = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
    return out, grads


def fixture_case(ref, case, live):
    fx = np.load(os.path.join(HERE, "pretrain_%s.npz" % case))
    samples = torch.from_numpy(fx["samples"])
    mask = torch.from_numpy(fx["mask_e200"]).bool()
    snap = bn_state(ref)
    res = {}
    for amp in (False, True):
        restore(ref, snap)
        act, grads = run_step(ref, samples, mask, fx["droppath_masks"], amp)
        bn = {k: ref.state_dict()[k].clone() for k in snap if "running" in k}
        res[amp] = act, grads, bn
    restore(ref, snap)
    act, grads, bn = res[False]
    # the fp32 run IS the existing fixture: every stored activation / gradient / BN statistic bit for bit
    assert sorted(grads) == sorted(live), "live-parameter set differs from the manifest"
    for k in fx.files:
        if k in act and k != "neighborhood":
            assert np.array_equal(act[k].astype(fx[k].dtype), fx[k]), (case, k)
        elif k.startswith("grad::"):
            g = grads[k[6:]]
            assert np.array_equal((g if g.numel() <= 65536 else g[:24]).numpy(), fx[k]), (case, k)
        elif k.startswith("gradnorm::"):
            assert float(grads[k[10:]].double().norm()) == float(fx[k]), (case, k)
        elif k.startswith("bn_after::"):
            assert np.array_equal(bn[k[10:]].numpy(), fx[k]), (case, k)
    gsq = sum(float(g.double().pow(2).sum()) for g in grads.values())
    assert gsq ** 0.5 == float(fx["grad_norm"]), case

    act16, grads16, bn16 = res[True]
    assert np.array_equal(act16["neighborhood"], act["neighborhood"]), "grouping must not depend on autocast"
    out = grad_arrays(grads, grads16, live)
    for k in ACT_KEYS:
        out["ac_err::" + k] = np.array(rel_l2(act16[k], act[k]))
    for k in sorted(bn):
        out["ac_err::bn_after::" + k] = np.array(rel_l2(bn16[k], bn[k]))
    for name in GRAD_SAMPLED:
        g, g16 = sample(grads[name]), sample(grads16[name])
        scale = float(g.abs().max())
        out["grad_scale::" + name] = np.array(scale)
        out["grad_sample::" + name] = (g / scale).numpy().astype(np.float16)
        out["ac_abs_sample::" + name] = np.array(float((g16 - g).norm()))
    return {case + "/" + k: v for k, v in out.items()}


def grad_arrays(grads, grads16, live):
    norm = np.array([float(grads[n].double().norm()) for n in live])
    err = np.array([float((grads16[n].double() - grads[n].double()).norm()) for n in live])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(norm > 0, err / np.where(norm > 0, norm, 1.0), np.nan)
    return {"gradnorm_all": norm, "ac_err_grad": rel, "ac_abs_grad": err}


def sample(g):
    """A weight (gradient) viewed as 2-D [out, in] -> every SAMPLE-th row and column, float64."""
    return g.detach().reshape(g.shape[0], -1)[::SAMPLE, ::SAMPLE].double()


def b128_case(ref_mod, live):
    """ac_err at the bench size: a fresh det-filled model, DropPath off, epoch-0 mask from the injected noise."""
    torch.manual_seed(0)
    ref = ref_mod.mae_vit_base_patch16_dec512d8b(norm_pix_loss=False, vis_mask_ratio=0.0)
    R.det_fill_(ref, seed=0)
    for mod in ref.modules():
        if isinstance(mod, R.DropPath):
            mod.drop_prob = 0.0
    x = clouds.uniform(B128, 1024, B128_CLOUD_SEED)
    noise = torch.rand(B128, 64, generator=torch.Generator().manual_seed(B128_NOISE_SEED))
    mask = epoch0_mask(noise).bool()
    snap = bn_state(ref)
    res = {}
    for amp in (False, True):
        restore(ref, snap)
        res[amp] = run_step(ref, x, mask, None, amp, teacher_noaug=False)
    (act, grads), (act16, grads16) = res[False], res[True]
    assert sorted(grads) == sorted(live)
    out = grad_arrays(grads, grads16, live)
    for k in ("teacher_loss_pred", "matrix", "chamfer_mean", "loss_learn"):
        out["ac_err::" + k] = np.array(rel_l2(act16[k], act[k]))
    out["grad_norm"] = np.array(float(np.sqrt((out["gradnorm_all"] ** 2).sum())))
    return {"b128/" + k: v for k, v in out.items()}


def write_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp and order, so that equal arrays give equal bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def main():
    torch.set_num_threads(THREADS)
    install_absent_packages()
    sys.path.insert(0, REF)
    import json
    import models_mae_learn_loss as ref_mod  # the reference file itself
    live = json.load(open(os.path.join(HERE, "state_dict_manifest.json")))["live_parameters"]

    torch.manual_seed(0)
    ref = ref_mod.mae_vit_base_patch16_dec512d8b(norm_pix_loss=False, vis_mask_ratio=0.0)
    R.det_fill_(ref, seed=0)
    out = {"param_names": np.array(live), "sample_stride": np.array(SAMPLE)}
    for case in CASES:
        out.update(fixture_case(ref, case, live))
        e = out[case + "/ac_err_grad"]
        print(case, "ac_err: chamfer %.2e  loss_learn %.2e  student_features %.2e  gradients median %.2e" % (
            out[case + "/ac_err::chamfer_mean"], out[case + "/ac_err::loss_learn"], out[case + "/ac_err::student_features"],
            float(np.nanmedian(e))))
    del ref
    out.update(b128_case(ref_mod, live))
    print("b128 ac_err: loss_pred %.2e  matrix %.2e  chamfer %.2e  gradients median %.2e" % (
        out["b128/ac_err::teacher_loss_pred"], out["b128/ac_err::matrix"], out["b128/ac_err::chamfer_mean"],
        float(np.nanmedian(out["b128/ac_err_grad"]))))
    path = os.path.join(HERE, "pretrain_bf16.npz")
    write_npz(path, out)
    print("wrote %s: %d keys, %.2f MB" % (path, len(out), os.path.getsize(path) / 2 ** 20))


if __name__ == "__main__":
    main()

"""CPU: the comparison helpers of tests/parity.py do what the bf16 parity tests rely on -- bf16-sized noise spread over a tensor
passes, one wrong (cloud, head) tile of the size the round-4 attn_qkv_fwd race produced is flagged (a whole-tensor band is not
moved by it), a uniform 5 % scale error fails rel-L2 -- and pretrain_bf16.npz covers every live parameter."""
import json
import os

import numpy as np
import pytest
import torch

from tests.parity import Ledger, cosine, rel_l2, tile_scores

GOLD = os.path.join(os.path.dirname(__file__), "golden")
AC_ERR = 1.2e-2         # the reference's own bf16-autocast error of the student features (pretrain_bf16.npz)


def _features(B=128, T=64, C=384, seed=0):
    """LayerNorm-output-like activations [B, T, C] and a bf16 computation of them: ~1 % relative error, then rounded to bf16."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(B, T, C, generator=g, dtype=torch.float64) * (0.8 + 0.4 * torch.rand(C, generator=g, dtype=torch.float64))
    got = (ref * (1 + AC_ERR * torch.randn(B, T, C, generator=g, dtype=torch.float64))).to(torch.bfloat16).double()
    return got, ref


def test_bf16_noise_passes():
    got, ref = _features()
    led = Ledger("noise")
    led.rel("features", got, ref, 3 * AC_ERR)
    led.cos("features", got, ref, 0.999)
    led.tiles("features", got, ref, "act", floor=1e-3)
    led.assert_ok()
    assert led.max_ratio() < 0.5            # with room: a correct computation is not near the bars


@pytest.mark.parametrize("B", [2, 128])
def test_one_wrong_head_tile_is_flagged(B):
    got, ref = _features(B=B)
    bad = got.clone()
    sign = torch.randint(0, 2, (64, 64), generator=torch.Generator().manual_seed(1)).double() * 2 - 1
    bad[B // 2, :, 128:192] += 0.2 * sign                       # one (cloud, head) tile off by 0.2, like the attn_qkv race
    if B == 128:    # 1/768 of the tensor: the 3 x ac_err rel-L2 bar (let alone the old 3 % loss band) lets it through
        assert rel_l2(bad, ref) <= 3 * AC_ERR and cosine(bad, ref) > 0.999
    scores = tile_scores(bad, ref, "act")
    assert scores[0][1] == "cloud %d cols 128:192" % (B // 2) and scores[0][0] > 1.0, scores[:3]
    led = Ledger("tile")
    led.tiles("features", bad, ref, "act", floor=1e-3)
    with pytest.raises(AssertionError, match=r"features tile cloud %d cols 128:192" % (B // 2)):
        led.assert_ok()


def test_one_wrong_weight_tile_is_flagged():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(1152, 384, generator=g, dtype=torch.float64) * 1e-3
    got = ref * (1 + 2e-2 * torch.randn(1152, 384, generator=g, dtype=torch.float64))
    assert tile_scores(got, ref, "weight")[0][0] < 0.5
    got[640:704, 64:128] *= 1.5                                  # one 64 x 64 block of a weight gradient 50 % off
    s = tile_scores(got, ref, "weight")
    assert s[0][1] == "[640:704, 64:128]" and s[0][0] > 1.0
    # the fixture's every-4th-row-and-column sample still sees it, and names the block in the weight's coordinates
    s = tile_scores(got[::4, ::4], ref[::4, ::4], "weight", stride=4)
    assert s[0][1] == "[640:704, 64:128]" and s[0][0] > 1.0 and s[1][0] < 0.5


def test_scaled_tensor_fails_rel_l2():
    got, ref = _features(B=8)
    led = Ledger("scale")
    led.rel("features", got * 1.05, ref, 3 * AC_ERR)
    led.tiles("features", got * 1.05, ref, "act")                # uniform: not localized
    assert led.rows[1][0] <= 1.0
    with pytest.raises(AssertionError, match="features rel-L2"):
        led.assert_ok()
    assert cosine(got * 1.05, ref) > 0.999                       # a pure scale error is invisible to the cosine


def test_ledger_names_the_six_worst():
    led = Ledger("t")
    for i in range(10):
        led.add("tensor%d" % i, i, 4.0)
    msg = led.report()
    assert all("tensor%d" % i in msg for i in range(4, 10)) and "tensor3" not in msg
    with pytest.raises(AssertionError, match="5 of 10 checks over their bar"):
        led.assert_ok()
    led = Ledger("nan")
    led.add("x", float("nan"), 1.0)
    with pytest.raises(AssertionError):
        led.assert_ok()


def test_bf16_fixture_schema():
    """pretrain_bf16.npz: every live parameter of the manifest has its fp32 norm and reference autocast error, per case."""
    live = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["live_parameters"]
    gold = np.load(os.path.join(GOLD, "pretrain_bf16.npz"))
    assert [str(n) for n in gold["param_names"]] == live and len(live) == 251
    for case in ("b2_uniform", "b4_gaussian", "b128"):
        norms, rel, ab = gold[case + "/gradnorm_all"], gold[case + "/ac_err_grad"], gold[case + "/ac_abs_grad"]
        assert norms.shape == rel.shape == ab.shape == (251,)
        assert np.isfinite(norms).all() and np.isfinite(ab).all() and (ab > 0).all()
        ok = norms > 0
        assert np.isfinite(rel[ok]).all() and np.allclose(rel[ok], ab[ok] / norms[ok])
        # the autocast errors are bf16-sized where the gradient is not analytically zero
        real = norms > 1e-5 * np.sqrt((norms ** 2).sum())
        assert 3e-3 < float(np.median(rel[real])) < 5e-2 and float(rel[real].max()) < 0.2
        acts = ("matrix", "chamfer_mean", "loss_learn") + (("teacher_loss_pred",) if case == "b128" else (
            "teacher_features", "teacher_noaug", "teacher_pix_pred", "teacher_loss_pred", "student_features", "student_pix_pred",
            "student_loss_pred"))
        for k in acts:
            assert 0 < float(gold[case + "/ac_err::" + k]) < 5e-2, (case, k)
    for case in ("b2_uniform", "b4_gaussian"):
        fx = np.load(os.path.join(GOLD, "pretrain_%s.npz" % case))
        i = {n: j for j, n in enumerate(live)}
        for k in fx.files:
            if k.startswith("gradnorm::"):                            # the fp32 fixture's own norms, same run
                assert float(gold[case + "/gradnorm_all"][i[k[10:]]]) == float(fx[k]), k
            if k.startswith("bn_after::"):
                assert case + "/ac_err::" + k in gold.files, k
        assert abs(np.sqrt((gold[case + "/gradnorm_all"] ** 2).sum()) - float(fx["grad_norm"])) <= 1e-9 * float(fx["grad_norm"])
    manifest = json.load(open(os.path.join(GOLD, "state_dict_manifest.json")))["state_dict"]
    stride = int(gold["sample_stride"])
    for case in ("b2_uniform", "b4_gaussian"):
        sampled = [k for k in gold.files if k.startswith(case + "/grad_sample::")]
        assert len(sampled) == 7
        for k in sampled:
            name = k.split("::", 1)[1]
            shape = manifest[name]
            assert gold[k].shape == (-(-shape[0] // stride), -(-int(np.prod(shape[1:])) // stride)), k
            assert gold[k].dtype == np.float16 and float(np.abs(gold[k]).max()) == 1.0
            assert float(gold[case + "/ac_abs_sample::" + name]) > 0

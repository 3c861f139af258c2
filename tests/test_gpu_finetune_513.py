"""-m gpu: the 8k fine-tune recipe's model half -- PointTransformer with 512 groups of 32, i.e. 513 tokens with the class token, one
token past what the LDS-resident attention kernels hold -- on the streaming kernels (gm3d_amd/csrc/attention_long.hip).

 * fp32: logits and the gradients of four parameters (the class token, the first block's qkv weight, the last block's fc2 weight, the
   embed's first convolution) against oracle/finetune_ref.py with the same state dict.  Logits and the three transformer gradients:
   within 1e-5 of the reference tensor's own maximum.  encoder.first_conv.0.weight alone: the gradient line of
   tests/test_gpu_finetune.py::test_step_against_oracle (2e-4 * max|g| + 1e-5 * the norm of the whole gradient) -- the embed's
   gradient passes two max-pools whose near-ties fall differently under another summation order, the embed is the same at any
   token count, and that line's 2e-4 term exists for it.  Measured on the MI355X, relative to each tensor's own max|g|: logits
   9.0e-7, cls_token 2.5e-6, qkv 1.1e-6, fc2 1.1e-6, first_conv 2.4e-4.
   This comparison runs eval-mode BatchNorm (see the test).  The train-mode head and embed at 512 groups of 32 are therefore covered
   only by the bf16 eager-vs-replay equality below, which has no reference: a gap.
 * bf16: one finetune_step with the flat optimizer, launched eagerly and replayed through GraphedFinetuneStep: loss and the updated
   flat parameters equal bit for bit.
Before the streaming kernels the constructor raised NotImplementedError for num_group + 1 > 512."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import finetune_ref as FR
from oracle import model_ref as R
from tests import clouds
from tests.test_gpu_finetune import CFG
from tests.test_gpu_model import rel

pytestmark = pytest.mark.gpu
CFG513 = dict(CFG, num_group=512, group_size=32, drop_path_rate=0.0)
PARAMS = ("cls_token", "blocks.blocks.0.attn.qkv.weight", "blocks.blocks.11.mlp.fc2.weight", "encoder.first_conv.0.weight")


def build(seed):
    from gm3d_amd.point_transformer import PointTransformer
    torch.manual_seed(0)
    m = PointTransformer(dict(CFG513))
    R.det_fill_(m, seed=seed)
    for mod in m.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    return m.cuda()


def test_fp32_forward_backward_against_oracle():
    """Eval-mode BatchNorm on both sides: with B = 2 a train-mode BatchNorm of the head normalises over TWO rows, which no fp32
    arithmetic holds to 1e-5 -- the oracle in fp32 is itself 6.6e-5 (logits) and 1e-3 (these gradients) away from the oracle in fp64
    there, against 8e-7 and 2.1e-6 with the running statistics (measured on the CPU).  In eval mode with gradients the token embed
    runs on its per-op modules (Encoder.fused); the block stack, the position embedding and the head stay on their fused paths."""
    pm = build(seed=5)
    om = FR.PointTransformer(drop_path_rate=0.0, num_group=512, group_size=32)
    om.load_state_dict({k: v.detach().cpu() for k, v in pm.state_dict().items()})
    for mod in om.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    om.eval(); pm.eval()
    pts = clouds.gaussian(2, 2048, seed=61)
    targets = torch.tensor([3, 17])
    ologits = om(pts.clone())
    nn.functional.cross_entropy(ologits, targets).backward()
    logits = pm(pts.clone().cuda())
    assert tuple(logits.shape) == (2, CFG["cls_dim"])
    nn.functional.cross_entropy(logits, targets.cuda()).backward()
    og, pg = dict(om.named_parameters()), dict(pm.named_parameters())
    ognorm = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in om.parameters())))
    err = {k: float((pg[k].grad.double().cpu() - og[k].grad.double()).abs().max()) for k in PARAMS}
    print("\nFT513 logits=%.2e gnorm=%.3e " % (rel(logits, ologits), ognorm)
          + " ".join("%s: %.2e of gnorm, %.2e of max|g|" % (k, err[k] / ognorm, rel(pg[k].grad, og[k].grad)) for k in PARAMS))
    assert rel(logits, ologits) <= 1e-5
    for k in PARAMS[:3]:
        assert rel(pg[k].grad, og[k].grad) <= 1e-5, (k, rel(pg[k].grad, og[k].grad))
    k = PARAMS[3]         # the embed: the gradient line of test_step_against_oracle, verbatim (two max-pools, see above)
    assert err[k] <= 2e-4 * float(og[k].grad.abs().max()) + 1e-5 * ognorm, (k, err[k], ognorm)


def test_bf16_flat_step_graph_replay_equals_eager():
    from gm3d_amd import engine_finetune as EF
    crit = nn.CrossEntropyLoss()
    warm, batch = (clouds.gaussian(2, 2048, seed=70 + i).cuda() for i in range(2))
    targets = torch.tensor([3, 17]).cuda()

    def run(graphed):
        pm = build(seed=9)
        pm.train()
        opt = EF.build_optimizer(pm, lr=1e-4, flat=True, max_norm=10.0)
        rng = np.random.RandomState(7)
        if graphed:      # the three warm-up iterations are real steps on the example batch: the eager side takes the same three
            step = EF.GraphedFinetuneStep(pm, crit, opt, warm, targets, npoints=2048, max_norm=10.0, bf16=True, rng=rng,
                                          augment=False, warmup_iters=3)
            loss = step(batch, targets)["loss"]
        else:
            sub = rng.choice(2048, 2048, False)
            for _ in range(3):
                EF.finetune_step(pm, crit, opt, warm, targets, npoints=2048, max_norm=10.0, bf16=True, subset=sub, augment=False)
            loss = EF.finetune_step(pm, crit, opt, batch, targets, npoints=2048, max_norm=10.0, bf16=True,
                                    subset=rng.choice(2048, 2048, False), augment=False)["loss"]
        torch.cuda.synchronize()
        return loss.detach().clone(), opt.P.detach().clone()

    le, pe = run(False)
    lg, pg = run(True)
    assert bool(torch.isfinite(le)) and bool(torch.isfinite(pe).all())
    assert torch.equal(le, lg), (float(le), float(lg))
    assert torch.equal(pe, pg)

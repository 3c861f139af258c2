"""Run-to-run identical results while the GPU is shared: the same launches repeated beside a concurrent load must give the same
bits as on a quiet card.  Round 4 found two kernels that did not (a wait sunk below an s_barrier in the fused qkv + attention kernel: any
concurrent load; FPS's long-lived LDS copy of the cloud: only beside another PROCESS, as in the two-rank tests).  These are the regression
tests; tools/replay_stress.py, op_stress.py, kernel_stress.py and fps_shared_gpu_probe.py are the long forms."""
import os
import subprocess
import sys
import threading
import time
from types import SimpleNamespace

import pytest
import torch

from tests import clouds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _segmented_step(B):
    from gm3d_amd import engine_pretrain as E, models_mae_learn_loss as M
    args = SimpleNamespace(mask_ratio=0.6, epochs=400, relative=True, bf16=True, accum_iter=1, lr=2e-4, min_lr=0.0, warmup_epochs=40)
    data = clouds.gaussian(B, 1024, 900).cuda()
    noise = torch.rand(B, 64, generator=torch.Generator().manual_seed(950)).cuda()
    torch.manual_seed(100)
    m = M.mae_vit_base_patch16_dec512d8b().cuda().train()
    for mod in m.modules():
        if isinstance(mod, M.DropPath):
            mod.drop_prob = 0.0
    ema = E.ModelEma(m, 0.999)
    opt = E.build_optimizer(m, lr=2e-4, flat=True, model_ema=ema, segment_of=E.ddp_segment)
    E.adjust_learning_rate(opt, 200.0, args)
    seg = E.SegmentedDDPStep(m, ema, opt, args, data, 200, warmup_iters=2, augment=False, inject_mask_noise=True, broadcast=False)
    seg.static_noise.copy_(noise)
    return seg, opt, data


def _replays_equal(seg, opt, n):
    """n replays of the three backward graphs (no optimizer step: the parameters stay put) -> how many differ from the first"""
    for g in seg.graphs[:3]:
        g.replay()
    torch.cuda.synchronize()
    ref = opt.G.detach().clone()
    bad = 0
    for i in range(n):
        opt.G.fill_(float("nan")) if i % 2 else opt.G.zero_()
        for g in seg.graphs[:3]:
            g.replay()
        torch.cuda.synchronize()
        bad += int(not torch.equal(opt.G, ref))
    return bad


def test_replays_identical_beside_a_second_stream_of_this_process():
    from gm3d_amd import attention, ops
    seg, opt, data = _segmented_step(64)
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda", dtype=torch.bfloat16)
    h = torch.randn(64 * 64, 384, device="cuda").bfloat16()
    wqkv = (torch.randn(1152, 384, device="cuda") * 0.05).bfloat16()
    xyz = data.contiguous()
    stop = []

    def busy():
        torch.cuda.set_device(0)
        with torch.cuda.stream(side):
            while not stop:
                for _ in range(10):
                    (big @ big).relu_()
                    ops.fps(xyz, 64)
                    attention.qkv_fwd(h, wqkv, 64, 64, 6, 0.125)
                side.synchronize()

    th = threading.Thread(target=busy)
    th.start()
    try:
        time.sleep(0.5)
        bad = _replays_equal(seg, opt, 250)
    finally:
        stop.append(1)
        th.join()
    assert bad == 0, "%d of 250 replays differed under a same-process load" % bad


def test_fps_identical_beside_another_process(tmp_path):
    """the situation of the two-rank tests: another process runs the same model's kernels on this GPU.  (Whole-step replays beside a
    loader process are the long form, tools/replay_stress.py: 0 of 5000 differ; they are not repeated here.)"""
    from gm3d_amd import ops
    xyz = clouds.gaussian(128, 1024, 901).cuda().contiguous()
    ref = ops.fps(xyz, 64)
    torch.cuda.synchronize()
    ready, stopf = str(tmp_path / "ready"), str(tmp_path / "stop")
    env = dict(os.environ, READY_FILE=ready, STOP_FILE=stopf)
    child = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "replay_stress.py"), "--load", "64", "120"], env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        t0 = time.time()
        while not os.path.exists(ready):
            assert child.poll() is None, "the loader process died: " + child.stdout.read().decode()[-2000:]
            assert time.time() - t0 < 300, "the loader process never became ready"
            time.sleep(0.5)
        bad_fps = 0
        for _ in range(3000):                    # the round-3 kernel: 3.5 % of launches differ beside a second process
            got = ops.fps(xyz, 64)
            torch.cuda.synchronize()
            bad_fps += int(not (torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])))
    finally:
        open(stopf, "w").write("stop")
        try:
            child.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            child.kill()
    assert bad_fps == 0, "%d of 3000 FPS launches differed beside a second process" % bad_fps

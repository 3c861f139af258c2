"""-m gpu: data-parallel Point-M2AE pretraining with TWO ranks (point_m2ae.SegmentedM2AEStep, engine_pretrain_m2ae.train_one_epoch
with world 2).  The test starts two fresh rank processes itself (tests/m2ae_ddp_worker.py); they share cuda:0 and gloo carries the
collectives.  B = 4 clouds of 2048 points per rank, bf16.

Checked: (1) ranks start from different seeds and are equal after construction; (2) after one step the averaged flat gradient is
identical on both ranks and EQUALS the mean of the two eagerly computed shard gradients (per-rank BatchNorm batch statistics, no
SyncBN); (3) parameters and teacher stay bit-identical across ranks after 3 steps; (4) the captured trajectory equals the eager
one; (5) one short train_one_epoch with world 2 ends with bit-identical replicas."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("m2ae_ddp"))
    port = _free_port()
    procs = []
    for r in range(2):
        log = open(os.path.join(out, "rank%d.log" % r), "w")
        procs.append((subprocess.Popen([sys.executable, "-m", "tests.m2ae_ddp_worker", "--rank", str(r), "--world", "2", "--port",
                                        str(port), "--out", out], cwd=ROOT, stdout=log, stderr=subprocess.STDOUT), log))
    rc = []
    try:
        for p, _ in procs:
            rc.append(p.wait(timeout=900))
    except subprocess.TimeoutExpired:
        rc = None
    finally:
        for p, log in procs:                 # only our own children
            if p.poll() is None:
                p.kill()
                p.wait()
            log.close()
    return {"dir": out, "rc": rc}


def _load(ranks, mode):
    d, logs = ranks["dir"], ""
    for r in range(2):
        for name in ("error_rank%d.txt" % r, "rank%d.log" % r):
            f = os.path.join(d, name)
            if os.path.exists(f):
                logs += "\n--- %s ---\n%s" % (name, open(f).read()[-3000:])
    assert ranks["rc"] == [0, 0], "worker exit codes %s%s" % (ranks["rc"], logs)
    return [torch.load(os.path.join(d, "%s_rank%d.pt" % (mode, r)), weights_only=True) for r in range(2)]


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_two_rank_segmented_m2ae_step(ranks, mode):
    r0, r1 = _load(ranks, mode)
    assert torch.equal(r0["p_start"], r1["p_start"])                                     # (1)
    assert torch.equal(r0["g_avg"], r1["g_avg"]) and not torch.equal(r0["g_local"], r1["g_local"])     # (2)
    # gloo sums the two buffers (one rounding), the step halves the sum (exact): the mean computed here, bit for bit
    want = (r0["g_local"] + r1["g_local"]) / 2
    for seg, (lo, hi) in r0["segments"].items():
        assert torch.equal(r0["g_avg"][lo:hi], want[lo:hi]), (mode, seg, float((r0["g_avg"][lo:hi] - want[lo:hi]).abs().max()))
    assert torch.equal(r0["params"], r1["params"]) and not torch.equal(r0["params"], r0["p_start"])    # (3)
    assert torch.equal(r0["ema"], r1["ema"])
    for a, b in zip(r0["losses"], r1["losses"]):
        assert all(x == x for x in a + b)
        assert a[2] == b[2]              # the gradient norm is of the averaged gradient: the same on both ranks


def test_two_rank_m2ae_graph_equals_eager(ranks):
    e0, _ = _load(ranks, "eager")
    g0, _ = _load(ranks, "graph")
    assert e0["losses"] == g0["losses"], (e0["losses"], g0["losses"])
    assert torch.equal(e0["g_avg"], g0["g_avg"])
    assert torch.equal(e0["params"], g0["params"]) and torch.equal(e0["ema"], g0["ema"])


def test_two_rank_m2ae_train_one_epoch(ranks):
    e0, e1 = _load(ranks, "epoch")
    assert torch.equal(e0["params"], e1["params"]) and torch.equal(e0["ema"], e1["ema"])
    for st in (e0["stats"], e1["stats"]):
        assert st["replayed_iters"] == 2 and st["capture_s"] > 0
        assert all(v == v and abs(v) != float("inf") for v in st.values())
    assert e0["stats"]["loss"] == e1["stats"]["loss"]           # the epoch's metric all-reduce

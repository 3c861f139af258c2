"""Throughput of the Point-M2AE classifier's fine-tune iteration (Point-M2AE_SA3D/cfgs/finetune_modelnet_PointM2AE.yaml: B = 40
clouds of 8192 points -> npoints 1024, 40 classes, bf16), eager / hipGraph replay / replay with the point sampling overlapped, each
with the fused classification tail (gm3d_cls_tail_*) and with the aten tail (point_m2ae_cls.FUSED_TAIL = False).

    python tools/bench_m2ae_finetune.py [--batch 40] [--steps 20] [--fp32] [--variant fused_graph]     (GPU box; one JSON line)

Launches per step: run ONE variant under `rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/bench_m2ae_finetune.py
--variant <name> --profile`; the timed steps are bracketed by two spin kernels (torch.cuda._sleep).  Then
`python tools/bench_m2ae_finetune.py --count <dir>/.../run_kernel_trace.csv --steps K` prints the dispatches per step between the
brackets, and those of them that are library GEMMs or PyTorch's generic reduction (reduce_kernel)."""
import argparse
import csv
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=40)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--points", type=int, default=8192)
ap.add_argument("--fp32", action="store_true")
ap.add_argument("--variant", default=None, help="run only this variant (e.g. fused_graph, aten_eager)")
ap.add_argument("--profile", action="store_true", help="bracket the timed steps with spin kernels (for --count)")
ap.add_argument("--count", default=None, help="a rocprofv3 kernel_trace.csv: print launches per step and exit")
a = ap.parse_args()

LIBRARY = ("Cijk", "hipblaslt", "rocblas", "gemm_kernel", "reduce_kernel")


def count(path, steps):
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r.get("Kernel_Name") or r.get("KernelName") or ""
    start = lambda r: int(r.get("Start_Timestamp") or r.get("BeginNs") or 0)
    rows.sort(key=start)
    marks = [i for i, r in enumerate(rows) if "spin" in name(r).lower() or "sleep" in name(r).lower()]
    if len(marks) < 2:
        raise SystemExit("no spin-kernel brackets in %s (run with --profile)" % path)
    inside = [name(r) for r in rows[marks[0] + 1:marks[-1]]]
    lib = sorted({n for n in inside if any(k.lower() in n.lower() for k in LIBRARY)})
    print(json.dumps({"launches_per_step": len(inside) / steps, "launches": len(inside), "steps": steps,
                      "library_or_reduce_kernels": lib}))


if a.count:
    count(a.count, a.steps)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from gm3d_amd import engine_finetune as EF  # noqa: E402
from gm3d_amd import point_m2ae_cls as C  # noqa: E402
from bench import make_clouds  # noqa: E402

dev = torch.device("cuda")
torch.manual_seed(0)
cfg = dict(NAME="Point_M2AE_ModelNet40", group_sizes=[16, 8, 8], num_groups=[512, 256, 64], encoder_depths=[5, 5, 5],
           encoder_dims=[96, 192, 384], local_radius=[0.32, 0.64, 1.28], drop_path_rate=0.1, num_heads=6, cls_dim=40)
crit = nn.CrossEntropyLoss()
args = SimpleNamespace(lr=5e-4, min_lr=1e-6, warmup_epochs=10, epochs=300)
pool = [make_clouds(a.batch, a.points, 100 + i, dev) for i in range(3)]
targets = (torch.arange(a.batch, device=dev) * 7) % 40
bf16 = not a.fp32
res = {}


def timed(step):
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    if a.profile:
        torch.cuda._sleep(1000)
    t0 = time.perf_counter()
    for i in range(a.steps):
        out = step(i)
    if a.profile:
        torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert np.isfinite(float(out["loss"]))
    return round(a.batch * a.steps / dt, 2), round(dt / a.steps * 1e3, 3)


def variant(tail, kind):
    C.FUSED_TAIL = tail == "fused"
    torch.manual_seed(0)
    model = C.build_model(cfg).to(dev).train()
    if kind == "eager":
        opt = EF.build_optimizer(model, lr=5e-4, flat=True, max_norm=10.0)

        def step(i):
            EF.adjust_learning_rate(opt, 20 + i / 100.0, args)
            return EF.finetune_step(model, crit, opt, pool[i % 3], targets, npoints=1024, bf16=bf16)
        return step
    opt = EF.build_optimizer(model, lr=5e-4, flat=True, max_norm=10.0)
    overlap = kind == "graph_overlap"
    g = EF.GraphedFinetuneStep(model, crit, opt, pool[0], targets, npoints=1024, max_norm=10.0, bf16=bf16, overlap_sampling=overlap)

    def step(i):
        EF.adjust_learning_rate(opt, 20 + i / 100.0, args)
        if overlap:
            return g(pool[i % 3], targets, next_points=pool[(i + 1) % 3])
        return g(pool[i % 3], targets)
    return step


for tail in ("fused", "aten"):
    for kind in ("eager", "graph", "graph_overlap"):
        name = "%s_%s" % (tail, kind)
        if a.variant and a.variant != name:
            continue
        try:
            res[name + "_clouds_per_s"], res[name + "_ms"] = timed(variant(tail, kind))
        except Exception as ex:       # a variant that cannot run is reported, the others still are
            res[name + "_error"] = "%s: %s" % (type(ex).__name__, str(ex)[:200])
C.FUSED_TAIL = True
res.update(metric="point-clouds/sec Point-M2AE fine-tune step (8192->1024 pts, cls 40, flat AdamW)", batch=a.batch,
           dtype="bf16" if bf16 else "f32", steps=a.steps)
print(json.dumps(res))

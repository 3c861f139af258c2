"""Writes tests/golden/gemm_bf16_bars.json: the GELU terms of the bars of tests/test_gpu_gemm_bf16_fp64.py, i.e. what an fp32 erf costs,
the one part of those bars that cannot be derived (tests/gemm_bf16_cases.py).  CPU only, a second:

    python tests/golden/make_gemm_bf16_bars.py

Per GELU-forward case and M: c = the largest |GELU_fp32(fl32(F + b)) - gelu64(F + b)| / (2^-24 |F + b|) over the case's own arguments
(F = the restated bf16 pre-activation of the graded inputs); per GELU-backward case and M: d = the largest
|GELU'_fp32(fl32(f + b)) - GELU'64(f + b)|, torch's autograd of its fp32 GELU.  The tests use 3 x these.  No figure here comes from a
kernel."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import gemm_bf16_cases as C      # noqa: E402


def gelu_row(c, M):
    x, w, b = C.tn_inputs("graded", M, c.N, c.K)
    f = C.tn_restate(x, w)
    a32, a64 = f.float() + b, f.double() + b.double()
    dist = (torch.nn.functional.gelu(a32).double() - C.gelu64(a64)).abs()
    ok = a64 != 0
    return {"c_gelu": float((dist[ok] / (2.0 ** -24 * a64[ok].abs())).max())}


def gelu_bwd_row(c, M):
    _, _, f, b = C.gelu_bwd_inputs(M, c.N, c.K)
    a32 = (f.float() + b).requires_grad_(True)
    torch.nn.functional.gelu(a32).sum().backward()
    return {"d_gelu_grad": float((a32.grad.double() - C.gelu_grad64(f.double() + b.double())).abs().max())}


def generate(verbose=False):
    table = {}
    for cases, row in ((C.GELU_CASES, gelu_row), (C.GELU_BWD_CASES, gelu_bwd_row)):
        for c in cases:
            for M in C.EPI_M:
                key = "%s-M%d" % (C.case_id(c), M)
                table[key] = row(c, M)
                if verbose:
                    print(key, table[key], flush=True)
    return table


if __name__ == "__main__":
    table = generate(verbose=True)
    with open(C.TABLE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")

"""Writes tests/golden/attention_long_bars.json: for every case of tests/attention_long_cases.py, how far the restatement of the case's
mode (mattn_ref.restate_f32 / emulate_bf16) is from the fp64 reference, per metric of mattn_ref.errors.  CPU only, a few minutes:

    python tests/golden/make_attention_long_bars.py

The GPU test's bar of a case is max(mattn_ref.BARS, 3 x this distance); tests/test_attention_long_cpu.py regenerates sampled rows."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import attention_long_cases as C      # noqa: E402


def row(c):
    return C.measure(c)


def generate(verbose=False):
    table = {}
    for c in C.cases():
        table[C.case_id(c)] = row(c)
        if verbose:
            print(C.case_id(c), " ".join("%s=%.2e" % kv for kv in sorted(table[C.case_id(c)].items())), flush=True)
    return table


if __name__ == "__main__":
    table = generate(verbose=True)
    with open(C.TABLE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")

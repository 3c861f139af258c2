"""Writes tests/golden/attention_plain_bars.json: for every case of tests/attention_plain_cases.py, how far the restatement of the
case's mode (mattn_ref.restate_f32 / emulate_bf16) is from the fp64 reference, per metric of mattn_ref.errors.  CPU only, one thread,
under a minute:

    python tests/golden/make_attention_plain_bars.py

A base case's bar is mattn_ref.BARS (tests/test_attention_plain_cpu.py: its row is at most half of it); the bar of an `amp` or `scale`
case is max(mattn_ref.BARS, 3 x this distance).  No figure here comes from a kernel."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import attention_plain_cases as C      # noqa: E402


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

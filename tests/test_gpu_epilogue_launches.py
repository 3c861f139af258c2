"""-m gpu: the launches of the three nodes whose products carry a fused epilogue, against the table recorded before gemm.py decided them.

tests/golden/epilogue_launches.json was written by tests/golden/make_golden_epilogue_launches.py on the GPU at the parent of the commit
that moved those decisions into gemm.route_gelu / route_gelu_bwd / route_pool / route_bn.  The same generator, run on the code under
test, must reproduce it launch for launch and integer for integer, in the same host order (the two lock-step inference chains
included); a case on one side only is a failure."""
import json

import pytest

from tests.golden import make_golden_epilogue_launches as E

pytestmark = pytest.mark.gpu


def test_every_case_launches_what_the_committed_table_lists():
    with open(E.PATH) as f:
        want = json.load(f)
    got = json.loads(E.dumps(E.generate()))
    assert list(want) == list(E.CASES), "the table and the generator's cases differ"
    assert list(got) == list(want)
    for k in want:
        first = next((i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b), min(len(got[k]), len(want[k])))
        assert got[k] == want[k], "%s: launch %d is %s, the table has %s (%d launches against %d)" % (
            k, first, got[k][first:first + 1], want[k][first:first + 1], len(got[k]), len(want[k]))

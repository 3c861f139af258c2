"""-m gpu: the launches of everything that runs attention, against the table recorded before gm3d_amd/attention.py decided them.

tests/golden/attention_launches.json was written by tests/golden/make_golden_attention_launches.py on the GPU at the parent of the
commit that moved the choice between the whole-head, LDS-resident, streaming, padded-streaming and qkv-fused launches into
attention.route / route_qkv.  The same generator, run on the code under test, must reproduce it launch for launch and integer for
integer, in the same host order (the two lock-step inference chains included); a case on one side only is a failure."""
import json

import pytest

from tests.golden import make_golden_attention_launches as A

pytestmark = pytest.mark.gpu


def test_every_case_launches_what_the_committed_table_lists():
    with open(A.PATH) as f:
        want = json.load(f)
    got = json.loads(A.E.dumps(A.generate()))
    assert list(want) == list(A.CASES), "the table and the generator's cases differ"
    assert list(got) == list(want)
    for k in want:
        first = next((i for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b), min(len(got[k]), len(want[k])))
        assert got[k] == want[k], "%s: launch %d is %s, the table has %s (%d launches against %d)" % (
            k, first, got[k][first:first + 1], want[k][first:first + 1], len(got[k]), len(want[k]))

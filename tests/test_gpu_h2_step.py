"""The h2 step lifecycle of tris_amd/ops.py, launch for launch: every case of tools/h2_step_trace.py issues the entry-point calls
recorded in tests/golden/h2_step_trace.json -- the same names with the same arguments in the same order, every amax word by the pool it
lies in and its index there (the tool's docstring) --, leaves the pool in the recorded state between them (the "#state" rows) and
computes the same bytes (the sha256 over its outputs and gradients, where the recording code itself repeated it).  The file was
recorded before the pool state became a declared record with named tags and is not regenerated from the code under test."""
import json

import pytest

from tools import h2_step_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(T.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases_of_the_tool(recorded):
    assert set(recorded) == set(T.CASES)
    assert sum(1 for r in recorded.values() if r["sha256"] is None) <= 2


@pytest.mark.parametrize("cid", list(T.CASES))
def test_launches_words_and_results_are_the_recorded_ones(recorded, cid):
    calls, digest = T.run_case(cid)
    got, want = json.loads(json.dumps(calls)), recorded[cid]["calls"]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{cid}: call {k} is {a}, recorded {b} (after {[c[0] for c in got[max(0, k - 3):k]]})"
    assert len(got) == len(want), f"{cid}: {len(got)} calls, recorded {len(want)}; the first one over: {max(got, want, key=len)[min(len(got), len(want))]}"
    if recorded[cid]["sha256"] is not None:
        assert digest == recorded[cid]["sha256"], f"{cid}: same launches, other bytes"

"""The BatchNorm dispatch of tris_amd/ops.py, launch for launch: every case of tools/bn_launch_trace.py issues the entry-point calls
recorded in tests/golden/bn_launch_trace.json -- the same names with the same arguments in the same order (pointers as null / non-null,
the tool's docstring).  The file was recorded before BatchNormFn was taken apart into named steps and is not regenerated from the
code under test."""
import json

import pytest

from tools import bn_launch_trace as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(T.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_the_cases_of_the_tool(recorded):
    assert set(recorded) == set(T.CASES)


@pytest.mark.parametrize("cid", list(T.CASES))
def test_launches_are_the_recorded_ones(recorded, cid):
    got, want = json.loads(json.dumps(T.run_case(cid))), recorded[cid]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"{cid}: call {k} is {a}, recorded {b} (after {[c[0] for c in got[max(0, k - 3):k]]})"
    assert len(got) == len(want), f"{cid}: {len(got)} calls, recorded {len(want)}; the first one over: {max(got, want, key=len)[min(len(got), len(want))]}"

"""Every refusal of the query entry points, held to what the library said before their argument checks were shared.

tests/refusal_cases.py is the matrix: per entry point a null context, n == 0, each pointer null, n = 0x80000000, each array misaligned,
each pair of arrays overlapping three ways, the call's own limits, and one probe per adjacent pair of steps of the checker that
breaks two rules at once.  tests/golden/query_refusals.json holds the return code and pt_last_error's text of every case, recorded by
tests/golden/make_refusals_golden.py; both must be reproduced exactly.

Nothing here has a scene: a call whose arguments pass is refused with "no scene (pt_set_scene first)", so a refusal lost by a mistake
is a failed comparison and never a launch.  Only the C ABI is used (ctypes), so the file runs on any build of the library.
"""
import json
import os

import pytest

import refusal_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_refusals.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    return {"refusals": refusal_cases.unpack(fixture), "tensor_messages": fixture["tensor_messages"]}


@pytest.fixture(scope="module")
def refusals():
    from acgpathtracing_amd import _native
    return refusal_cases.run_all(_native.hip())


def test_the_matrix_is_the_recorded_one(golden, refusals):
    assert sorted(golden["refusals"]) == sorted(refusals) == sorted(refusal_cases.BY_KEY)


@pytest.mark.parametrize("key", sorted(refusal_cases.BY_KEY))
def test_refusals_equal_the_recorded_ones(golden, refusals, key):
    want, got = golden["refusals"][key], refusals[key]
    assert sorted(want) == sorted(got)
    wrong = {label: (got[label], want[label]) for label in want if got[label] != want[label]}
    assert not wrong, wrong
    # the safety condition: what passes every argument check ends at the missing scene
    no_scene = [1, refusal_cases.BY_KEY[key].name + ": no scene (pt_set_scene first)"]
    if not refusal_cases.BY_KEY[key].posed:
        assert want["all arguments fine"] == no_scene
    else:
        assert want["all arguments fine"][1].endswith("no query mesh (pt_set_query_mesh first)")
        assert want["with a query mesh: all arguments fine"] == no_scene
        assert want["with a query mesh: too many posed triangles"][1].endswith("too many posed triangles (2^31 - 1 per call): split the poses")


def test_tensor_refusals_equal_the_recorded_ones(golden):
    """pathtracer.py's own refusals of a tensor (device, dtype, shape, contiguity, and what may not come with a tensor): the recorded
    message, raised before the library is called"""
    got = refusal_cases.run_tensor_messages()
    want = golden["tensor_messages"]
    assert sorted(got) == sorted(want) and "accepted" not in want.values()
    wrong = {label: (got[label], want[label]) for label in want if got[label] != want[label]}
    assert not wrong, wrong

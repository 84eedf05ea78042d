"""The C ABI's boundary against its recorded table (tests/abi_boundary_cases.py wrote tests/golden/abi_boundary.json): every refusal's return
code and text, and every valid call's workspace peak and results, are what they were when the table was recorded."""
import json
import os

import pytest

import abi_boundary_cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got():
    return abi_boundary_cases.run()


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "abi_boundary.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("purpose", ["full", "decoder"])
def test_refusals(got, want, purpose):
    g, w = got[purpose]["refusals"], want[purpose]["refusals"]
    assert sorted(g) == sorted(w), "the cases are not the recorded ones"
    assert len(w) > 100
    wrong = {case: (g[case], w[case]) for case in w if list(g[case]) != list(w[case])}
    assert not wrong, "%d of %d refusals differ (got, recorded): %r" % (len(wrong), len(w), wrong)


@pytest.mark.parametrize("purpose", ["full", "decoder"])
def test_valid_calls(got, want, purpose):
    g, w = got[purpose]["valid"], want[purpose]["valid"]
    assert sorted(g) == sorted(w) == sorted(abi_boundary_cases.ENTRIES), "the entries are not the recorded ones"
    wrong = {name: (g[name], w[name]) for name in w if g[name] != w[name]}
    assert not wrong, "%d of %d valid calls differ (got, recorded): %r" % (len(wrong), len(w), wrong)
    served = [name for name in w if w[name]["rc"] == 0]
    assert len(served) == (len(w) if purpose == "full" else sum("fwd" not in f for _, f in abi_boundary_cases.ENTRIES.values()))
    assert all(w[name]["crc32"] for name in served), "a served call that wrote nothing"

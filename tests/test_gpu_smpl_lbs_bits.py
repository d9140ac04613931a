"""The outputs of the eight C entry points of the SMPL / LBS family, bit for bit, against tests/golden/smpl_lbs_bits.json (the
SHA-256 of every output tensor, recorded once by tests/golden/make_golden_smpl_lbs_bits.py; its docstring lists the cases).  These
kernels form every sum in float64 in a fixed order: a change to the chain, to a fold order or to an operand order in ONE of several
copies passes every tolerance test and fails here.

The bits are the compiler's too: under another toolchain than the recorded one the comparison says nothing and the tests skip,
naming both."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_smpl_lbs_bits as gen  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(hip_lib):
    with open(gen.PATH) as f:
        doc = json.load(f)
    here = gen.toolchain()
    there = {k: doc[k] for k in here}
    if here != there:
        pytest.skip(f"smpl_lbs_bits.json was recorded under {there}, this is {here}: the bits are not comparable")
    return doc["cases"]


def test_the_file_holds_exactly_the_generator_s_cases():
    with open(gen.PATH) as f:
        assert sorted(json.load(f)["cases"]) == sorted(gen.case_names())


@pytest.mark.parametrize("name", gen.case_names())
def test_every_output_has_the_recorded_bits(recorded, gpu, name):
    got, want = gen.run_case(name, gpu), recorded[name]
    assert sorted(got) == sorted(want)
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{name}: {len(differ)} of {len(want)} outputs differ from the recorded bits: {differ}"

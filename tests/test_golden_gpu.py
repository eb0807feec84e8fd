"""GPU: the HIP slots through the C ABI reproduce tests/golden/ref_slots.json, the digests of what the reference decoder's own C
path computed on the case lists of tests/ref_cases.py: HIP against the reference with no oracle in between.  On a mismatch the
oracle runs the same group, so that the failure names the case and the first differing sample.  Reads only tests/golden/ and
the case module."""
import pytest

import ref_cases
import ref_lib
from golden_check import check_slot

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def golden():
    return ref_lib.load_golden()


PARAMS = [(slot, bd) for slot in ref_cases.DEVICE_SLOTS for bd in ref_cases.slot_bds(slot)]


@pytest.mark.parametrize("slot,bd", PARAMS, ids=[f"{s}-{b}" if b else s for s, b in PARAMS])
def test_hip_reproduces_reference_digests(dev, golden, slot, bd):
    def explain(cases, outs):
        orc = getattr(ref_lib.load_oracle(), "orc_" + slot)
        for c, got in zip(cases, outs):
            d = ref_cases.first_difference(c, ref_cases.outputs(c, *ref_cases.run(c, orc)), got)
            if d:
                return "HIP differs from the oracle: " + d
        return "HIP agrees with the oracle on every case of the group: the oracle differs from the reference here (tests/test_golden_cpu.py)"

    assert check_slot(golden, slot, getattr(dev, "vvc355_" + slot), bd=bd, explain=explain) > 0

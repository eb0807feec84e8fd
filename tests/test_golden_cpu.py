"""CPU, runs everywhere: the oracle reproduces tests/golden/ref_slots.json, the digests of what the reference's own C path
computed on the case lists of tests/ref_cases.py (tools/gen_golden.py).  A group whose inputs do not hash to the recorded
input digest fails with "generator drifted"; no group may be missing on either side; where the live reference is present the
committed file must equal a fresh generation."""
import os
import sys

import pytest

import ref_cases
import ref_lib
from golden_check import check_slot


@pytest.fixture(scope="module")
def golden():
    return ref_lib.load_golden()


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.mark.parametrize("slot", ref_cases.SLOTS)
def test_oracle_reproduces_reference_digests(golden, orc, slot):
    ref = ref_lib.load()

    def explain(cases, outs):          # with the live reference at hand, name the sample
        if ref is None:
            return "first cases " + "; ".join(str(c.params) for c in cases[:4])
        for c, got in zip(cases, outs):
            d = ref_cases.first_difference(c, ref_cases.outputs(c, *ref_cases.run(c, getattr(ref, "ref_" + slot))), got)
            if d:
                return d
        return "the live reference agrees with the oracle: the fixture is stale"

    n = check_slot(golden, slot, getattr(orc, "orc_" + slot), explain=explain)
    assert n == len(golden[slot])
    print(f"{slot}: {n} groups reproduced")


def test_no_group_left_out(golden):
    want = {slot: {gid.split("/", 1)[1] for gid, _ in ref_cases.groups(slot)} for slot in ref_cases.SLOTS}
    have = {slot: set(groups) for slot, groups in golden.items()}
    assert set(want) == set(have), f"slots differ: {sorted(set(want) ^ set(have))}"
    for slot in want:
        assert want[slot] == have[slot], f"{slot}: groups differ: {sorted(want[slot] ^ have[slot])[:8]}"
    print(f"{sum(len(v) for v in want.values())} groups in {len(want)} slots, none left out")


def test_fixture_is_fresh():
    lib = ref_lib.load()
    if lib is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(ref_lib.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps(gen_golden.generate(lib, "ref_")), "tests/golden/ref_slots.json is stale: python tools/gen_golden.py"

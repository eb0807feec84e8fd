"""CPU, runs everywhere: the oracle reproduces tests/golden/ref_slots.json, the digests of what the reference's own C path
computed on the case lists of tests/ref_cases.py (tools/gen_golden.py).  A group whose inputs do not hash to the recorded
input digest fails with "generator drifted"; no group may be missing on either side; where the live reference is present the
committed file must equal a fresh generation."""
import os
import sys

import pytest

import ctx_mirror
import ref_cases
import ref_ctx_cases
import ref_lib
from golden_check import check_ctx_slot, check_slot


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


@pytest.mark.parametrize("slot", ref_ctx_cases.SLOTS)
def test_host_shim_and_oracle_reproduce_reference_digests(golden, orc, slot):
    """The slots that take the decoder's context: the host shim's flattening, then the oracle's flat form (for the two availability
    functions the host shim alone), against the digests of the reference's real slots on real structs."""
    lib = ref_lib.load()

    def explain(cases, outs):
        if lib is None:
            return "first cases " + "; ".join(str(c.params) for c in cases[:4])
        side = ref_ctx_cases.reference_side(lib)
        for c, got in zip(cases, outs):
            d = ref_ctx_cases.first_difference(c, ref_ctx_cases.run(c, side), got)
            if d:
                return d
        return "the live reference agrees with the project: the fixture is stale"

    n = check_ctx_slot(golden, slot, ref_ctx_cases.oracle_side(orc, ctx_mirror.load_host()), explain=explain)
    assert n == len(golden[slot])
    print(f"{slot}: {n} groups reproduced")


def test_no_group_left_out(golden):
    want = {slot: {gid.split("/", 1)[1] for gid, _ in ref_cases.groups(slot)} for slot in ref_cases.SLOTS}
    want.update({slot: {gid.split("/", 1)[1] for gid, _ in ref_ctx_cases.groups(slot)} for slot in ref_ctx_cases.SLOTS})
    have = {slot: set(groups) for slot, groups in golden.items()}
    assert set(want) == set(have), f"slots differ: {sorted(set(want) ^ set(have))}"
    for slot in want:
        assert want[slot] == have[slot], f"{slot}: groups differ: {sorted(want[slot] ^ have[slot])[:8]}"
    print(f"{sum(len(v) for v in want.values())} groups in {len(want)} slots, none left out")


def test_regeneration_only_adds():
    """tools/gen_golden.py refuses a regeneration that changes or drops a recorded group: its check sees additions, and nothing else."""
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    old = {"a": {"8/0": ["i", "o"], "8/1": ["i", "p"]}}
    assert gen_golden.changed_digests(old, {"a": {"8/0": ["i", "o"], "8/1": ["i", "p"], "8/2": ["j", "q"]}, "b": {"0/0": ["k", "r"]}}) == []
    assert gen_golden.changed_digests(old, {"a": {"8/0": ["i", "x"], "8/1": ["i", "p"]}}) == ["a/8/0"]
    assert gen_golden.changed_digests(old, {"a": {"8/0": ["i", "o"]}}) == ["a/8/1"]
    assert gen_golden.changed_digests(old, {}) == ["a/8/0", "a/8/1"]


def test_fixture_is_fresh():
    lib = ref_lib.load()
    if lib is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(ref_lib.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps(gen_golden.generate(lib, "ref_")), "tests/golden/ref_slots.json is stale: python tools/gen_golden.py"

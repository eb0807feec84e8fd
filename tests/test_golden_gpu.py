"""GPU: the HIP slots through the C ABI reproduce tests/golden/ref_slots.json, the digests of what the reference decoder's own C
path computed on the case lists of tests/ref_cases.py: HIP against the reference with no oracle in between.  On a mismatch the
oracle runs the same group, so that the failure names the case and the first differing sample.  Reads only tests/golden/ and
the case module."""
import pytest

import ctx_mirror
import ref_cases
import ref_ctx_cases
import ref_lib
from golden_check import check_ctx_slot, check_slot

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


CTX_PARAMS = [(slot, bd) for slot in ref_ctx_cases.DEVICE_SLOTS for bd in ref_cases.BDS]


@pytest.mark.parametrize("slot,bd", CTX_PARAMS, ids=[f"{s}-{b}" for s, b in CTX_PARAMS])
def test_installed_table_reproduces_reference_digests(dev, golden, slot, bd):
    """The three slots that take the decoder's context, through the table ff_vvc_dsp_init_mi355_ctx installs and with the mirror
    context: the host shim and the kernel against the reference's real slot on real structs, with no oracle in between."""
    host = ctx_mirror.load_host()

    def explain(cases, outs):
        side = ref_ctx_cases.oracle_side(ref_lib.load_oracle(), host)
        for c, got in zip(cases, outs):
            d = ref_ctx_cases.first_difference(c, ref_ctx_cases.run(c, side), got)
            if d:
                return "the table's slot differs from the host shim + oracle: " + d
        return "the table's slot agrees with the host shim + oracle on every case of the group: they differ from the reference here (tests/test_golden_cpu.py)"

    assert check_ctx_slot(golden, slot, ref_ctx_cases.table_side(host), bd=bd, explain=explain) > 0


def test_derive_transform_type_whole_domain(dev):
    """The digests hold every 1009th tuple of derive_transform_type's domain (ref_cases.DIGEST_STRIDE); the oracle is compared with the
    live reference on all of them (tests/test_oracle_ref_cpu.py), and here the product's function, the one its kernels compile too, with
    the oracle on all of them: integer calls only."""
    orc = ref_lib.load_oracle().orc_derive_transform_type
    fn = dev.vvc355_derive_transform_type
    lst = ref_cases.cases("derive_transform_type")
    assert len(lst) == 256 * 5 * 3 * 3 * 7 * 7
    for c in lst:
        assert fn(*c.args) == orc(*c.args), c.params

"""Inter prediction, reconstruction and inverse LMCS of whole pictures pinned to the reference's own three calls per CTU, CPU side
(tests/ref_picture_cases.py has the pictures and both sides).

* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): on every listed picture W0-W9 and on 48 freshly drawn ones what
  ref_decode_picture leaves — the planes after ff_vvc_reconstruct, the planes after ff_vvc_lmcs_filter, tab_dmvr_mvf, the chroma scales
  the reference cached — equals the chained oracle (inter_oracle, ciip_oracle, a LUT lookup under lmcs_mask) fed the inputs derived by
  INTEGRATION.md section 3.  The shim's -1 fails the test: no picture is skipped, listed or drawn.  The premises that only the reference's
  outputs show are counted, the sensitivity table of ref_picture_cases.py is recomputed, and the shim's refusals are checked.
* Everywhere: the generator alone stays inside the domain (listed pictures and the sweep's draws), the premises are counted from the
  description, the oracle chain reproduces tests/golden/ref_picture.json, the inputs still hash to theirs, no picture is missing."""
import ctypes
import os
import sys
import time
from collections import Counter

import numpy as np
import pytest

import ref_lib
import ref_picture_cases as pc
import ref_recon_cases as rc
from ffvvc_amd import abi


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load()


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


def test_reference_library_has_the_entry_where_the_tree_is():
    if ref_lib.reference_tree() is None:
        pytest.skip("no reference tree on this machine")
    lib = ref_lib.load()
    assert lib is not None and hasattr(lib, "ref_decode_picture"), f"{ref_lib.LIB_PATH} has no ref_decode_picture"
    pc.bind_reference(lib)


def _compare(ref, orc, pic):
    """Reference and oracle chain compared whole; returns both results."""
    assert pc.in_domain(pic) is None, f"{pic.name}: {pc.in_domain(pic)}"
    r = pc.run_reference(ref, pic)
    assert r.ret == 0, f"{pic.name}: the shim refused the picture ({r.ret}): the generator left its domain"
    assert not r.twice, f"{pic.name}: the reference cached two different scales for the units at {r.twice[:4]}"
    o = pc.run_oracle(orc, pic)
    for what, want, got in (("after reconstruction", r.recon, o.recon), ("after inverse LMCS", r.final, o.final)):
        diff = rc.first_difference(want, got)
        assert diff is None, f"{pic.name}: reference / oracle chain {what}: {diff}"
    bad = np.argwhere((pc.mvf_bytes(r.dmvr) != pc.mvf_bytes(o.dmvr)).any(-1))
    assert not len(bad), f"{pic.name}: tab_dmvr_mvf: {len(bad)} entries differ, first at unit (row, col) {bad[0].tolist()}"
    d = o.d
    if o.table is not None:
        t = o.table.reshape(d.tpic.uy, d.tpic.ux)
        for (ux, uy) in d.routed:
            key = (ux * pic.size_y, uy * pic.size_y)
            assert key in r.scales, f"{pic.name}: the host routes unit {key} to the TB passes, the reference never asked for its scale"
            assert r.scales[key] == t[uy, ux], f"{pic.name}: unit {key}: the reference cached {r.scales[key]}, orc_lmcs_vpdu_scale_pass gives {t[uy, ux]}"
    else:
        assert not r.scales and not d.routed
    return r, o


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", pc.picture_names())
def test_live_picture_equals_the_reference(ref, orc, name):
    _need(ref)
    pic = pc.picture(name)
    r, _o = _compare(ref, orc, pic)
    assert any(np.any(a != b) for a, b in zip(r.recon, r.final)) == any(sl[1] for sl in pic.slices)


def test_live_sweep(ref, orc):
    _need(ref)
    t0, seen, units, n_ciip = time.time(), Counter(), 0, 0
    for k in range(pc.SWEEP):
        pic = pc.sweep_picture(k)
        _compare(ref, orc, pic)
        seen[(pic.bd, pic.idc, pic.ctb_log2)] += 1
        units += sum(len(c) for c in pic.ctus)
        n_ciip += len(pc.inputs(pic).e.ciip)
    assert sum(seen.values()) >= 48
    assert {k[0] for k in seen} == {8, 10, 12} and {k[1] for k in seen} == {0, 1, 2, 3} and {k[2] for k in seen} == {5, 6, 7}
    assert n_ciip > 200
    print(f"{pc.SWEEP} pictures ({units} units, {n_ciip} CIIP units) in {len(seen)} configurations compared in {time.time() - t0:.1f} s")


def test_live_premises_from_the_reference(ref):
    _need(ref)
    total = Counter()
    for name in pc.picture_names():
        pic = pc.picture(name)
        total.update(pc.census(pic, pc.run_reference(ref, pic)))
    missing = [p for p in pc.REFERENCE_PREMISES if not total[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"
    print({p: total[p] for p in pc.REFERENCE_PREMISES})


def test_live_sensitivity(ref, orc):
    """Each misreading, applied to the oracle side alone, is caught by the pictures the table names; the one that no picture catches has
    its reason in ref_picture_cases' docstring."""
    _need(ref)
    refs = {n: pc.run_reference(ref, pc.picture(n)) for n in pc.picture_names()}
    for mis in pc.MISREADINGS:
        fails = []
        for n in pc.picture_names():
            o, r = pc.run_oracle(orc, pc.picture(n), mis), refs[n]
            if rc.first_difference(r.recon, o.recon) or rc.first_difference(r.final, o.final) or not np.array_equal(pc.mvf_bytes(r.dmvr), pc.mvf_bytes(o.dmvr)):
                fails.append(n)
        assert fails == pc.SENSITIVITY[mis], f"'{mis}' is caught by {fails}: ref_picture_cases.SENSITIVITY and its docstring say {pc.SENSITIVITY[mis]}"
        assert fails or mis == "ciip_unit_in_the_regular_list", f"no listed picture catches '{mis}': a picture is missing"


def test_live_shim_refuses_what_its_objects_cannot_hold(ref):
    """A record with no unit at its origin, a unit with inter luma and no record, a CIIP unit in the regular list, slice flags that disagree."""
    _need(ref)
    pic = pc.picture("W0")
    i = pc.inputs(pic)
    assert len(i.e.inter) > 2 and len(i.e.ciip) > 2

    def moved(m, f, lists):
        lists.inter["x0"][0] += 4

    def dropped(m, f, lists):
        lists.gpm = lists.gpm[:-1]

    def ciip_as_regular(m, f, lists):
        c = lists.ciip[0]
        lists.inter[0]["x0"], lists.inter[0]["y0"], lists.inter[0]["cb_width"], lists.inter[0]["cb_height"] = c["x0"], c["y0"], c["cb_width"], c["cb_height"]
        lists.inter[0]["num_sb_x"], lists.inter[0]["num_sb_y"], lists.inter[0]["slice"] = 1, 1, c["slice"]

    def twice(m, f, lists):
        lists.ciip = np.concatenate([lists.ciip, lists.ciip[:1]])

    keep = []

    def slice_flags(m, f, lists):
        n = len(pic.slices)
        s = (abi.InterSlice * n).from_buffer_copy(ctypes.string_at(f.slices, ctypes.sizeof(abi.InterSlice) * n))
        s[0].lmcs_used ^= 1
        keep.append(s)
        f.slices = ctypes.addressof(s)

    for change in (moved, dropped, ciip_as_regular, twice, slice_flags):
        assert pc.run_reference(ref, pic, change).ret == -1, f"the shim took a picture with {change.__name__}"
    assert pc.run_reference(ref, pic).ret == 0


def test_live_fixture_is_fresh(ref):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(pc.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_picture(ref)), "tests/golden/ref_picture.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- everywhere

def test_generator_stays_inside_the_domain():
    """Listed pictures and every draw of the sweep, by the generator alone: no refusal can come from the description."""
    for pic in [pc.picture(n) for n in pc.picture_names()] + [pc.sweep_picture(k) for k in range(pc.SWEEP)]:
        assert pc.in_domain(pic) is None, f"{pic.name}: {pc.in_domain(pic)}"
        assert pic.width <= 264 and pic.height <= 136
        assert all(np.all(p == pic.sentinel) for p in pic.planes)
    for name in pc.picture_names():                      # what the device test asks of a listed picture: every stage has work
        e = pc.inputs(pc.picture(name)).e
        assert len(e.inter) and len(e.affine) and len(e.gpm) and len(e.ciip) > 5, f"{name}: a stage without a unit"


def test_premises_of_the_listed_pictures():
    total = Counter()
    for name in pc.picture_names():
        total.update(pc.census(pc.picture(name)))
    missing = [p for p in pc.PREMISES if not total[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"
    print({p: total[p] for p in pc.PREMISES})


@pytest.mark.parametrize("name", pc.picture_names())
def test_oracle_chain_reproduces_reference_digests(golden, orc, ref, name):
    assert name in golden, f"{name} is not in ref_picture.json: regenerate it (tests/golden/README.md)"
    got = pc.oracle_digests(orc, name)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle chain's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the first sample")


def test_no_picture_left_out(golden):
    assert list(golden) == pc.picture_names()
    assert set(pc.RASTER_TOO) <= set(golden) and set(pc.SENSITIVITY) == set(pc.MISREADINGS)

"""The RECON walk and the TB record passes pinned to ff_vvc_reconstruct, CPU side (tests/ref_recon_cases.py has the pictures and both
derivations).

* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): on every listed picture and on 48 freshly drawn ones the reference's
  planes, compared whole, equal the oracle side's — intra_tb_cases.oracle_block, the residuals and tails of the inter_tb_cases / ts_tb_cases
  walks, orc_lmcs_vpdu_scale_pass, orc_recon_frame_pass, fed the inputs derived by INTEGRATION.md's rules — and every chroma scale the
  reference cached for a unit whose blocks go to the TB passes equals that unit's table entry.  The shim's -1 fails the test: no picture is
  skipped.  The sensitivity table of ref_recon_cases.py is recomputed.
* Everywhere: the command lists are well-formed (vvc355_recon_order_check's rules, restated: the GPU test launches a picture only on lists this
  test has accepted), the oracle side reproduces tests/golden/ref_recon.json, the inputs still hash to theirs, no picture is missing, and
  the pictures reach what the pin is for (ref_recon_cases.PREMISES, counted)."""
import os
import sys
import time
from collections import Counter

import numpy as np
import pytest

import picture_cases as pcs
import ref_lib
import ref_recon_cases as rc

SWEEP = 48


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load()


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


def test_reference_library_has_the_entry_where_the_tree_is():
    if ref_lib.reference_tree() is None:
        pytest.skip("no reference tree on this machine")
    lib = ref_lib.load()
    assert lib is not None and hasattr(lib, "ref_recon_picture"), f"{ref_lib.LIB_PATH} has no ref_recon_picture"
    rc.bind_reference(lib)                              # the arrays' layout


def _compare(ref, orc, pic):
    d = rc.derive(pic)
    ret, want, scales, twice = rc.run_reference(ref, pic)
    assert ret == 0, f"{pic.name}: the shim refused the picture ({ret}): the generator left its domain"
    assert not twice, f"{pic.name}: the reference cached two different scales for the units at {twice[:4]}"
    got, table, _arena = rc.oracle_side(orc, d)
    diff = rc.first_difference(want, got)
    assert diff is None, f"{pic.name}: reference / oracle side: {diff}"
    if table is not None:
        t = table.reshape(d.tpic.uy, d.tpic.ux)
        for (ux, uy) in d.routed:
            key = (ux * pic.size_y, uy * pic.size_y)
            assert key in scales, f"{pic.name}: the host routes unit {key} to the TB passes, the reference never asked for its scale"
            assert scales[key] == t[uy, ux], f"{pic.name}: unit {key}: the reference cached {scales[key]}, orc_lmcs_vpdu_scale_pass gives {t[uy, ux]}"
    else:
        assert not scales and not d.routed
    return d, want, scales


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", rc.picture_names())
def test_live_reconstruction_equals_the_reference(ref, orc, name):
    _need(ref)
    pic = rc.picture(name)
    _d, want, _ = _compare(ref, orc, pic)
    assert any(np.any(w != p) for w, p in zip(want, pic.planes))


def test_live_sweep(ref, orc):
    _need(ref)
    t0, seen, n, units, routed, walked = time.time(), Counter(), 0, 0, 0, 0
    for k in range(SWEEP):
        pic = rc.sweep_picture(k)
        d, _want, _scales = _compare(ref, orc, pic)
        seen[(pic.bd, pic.idc, pic.ctb_log2)] += 1
        units += sum(len(c) for c in pic.ctus)
        routed += len(d.routed)
        walked += d.stats["walk_scaled"]
        n += 1
    assert n >= 48, n
    assert {k[0] for k in seen} == {8, 10, 12} and {k[1] for k in seen} == {0, 1, 2, 3} and {k[2] for k in seen} == {5, 6, 7}
    assert routed > 20 and walked > 20
    print(f"{n} pictures ({units} units, {routed} units scaled through the table, {walked} blocks scaled in the walk) in {len(seen)} configurations "
          f"compared in {time.time() - t0:.1f} s")


def test_live_reference_alone_accepts_every_picture(ref):
    """The domain check without the oracle: the reference takes all listed and drawn pictures, and leaves what it does not own alone."""
    _need(ref)
    for pic in [rc.picture(n) for n in rc.picture_names()] + [rc.sweep_picture(k) for k in range(SWEEP)]:
        ret, planes, _scales, twice = rc.run_reference(ref, pic)
        assert ret == 0 and not twice, (pic.name, ret, twice)
        owned = np.zeros((pic.height, pic.width), bool)
        for ctu in pic.ctus:
            for cu in ctu:
                if cu["coded_flag"]:
                    owned[cu["y0"]:cu["y0"] + cu["h"], cu["x0"]:cu["x0"] + cu["w"]] = True
        assert np.array_equal(planes[0][~owned], pic.planes[0][~owned]), f"{pic.name}: the reference wrote luma of an uncoded unit"


def test_live_shim_refuses_a_ciip_unit(ref):
    _need(ref)
    pic = rc.sweep_picture(0)
    cu = next(cu for ctu in pic.ctus for cu in ctu if cu["pred_mode"] == 0)
    try:
        cu["ciip_flag"], pic._flat = 1, None
        assert rc.run_reference(ref, pic)[0] == -1
    finally:
        cu["ciip_flag"], pic._flat = 0, None
    assert rc.run_reference(ref, pic)[0] == 0


def test_live_sensitivity(ref, orc):
    """Each misreading, applied to the derivation of the project's inputs alone, is caught by the pictures the table names, and by at least one."""
    _need(ref)
    refs = {n: rc.run_reference(ref, rc.picture(n))[1] for n in rc.picture_names()}
    for mis in rc.MISREADINGS:
        fails = [n for n in rc.picture_names() if rc.first_difference(refs[n], rc.oracle_side(orc, rc.derive(rc.picture(n), mis))[0])]
        assert fails, f"no listed picture catches '{mis}': a picture is missing"
        assert fails == rc.SENSITIVITY[mis], f"'{mis}' is caught by {fails}: ref_recon_cases.SENSITIVITY and its docstring say {rc.SENSITIVITY[mis]}"


def test_live_fixture_is_fresh(ref):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(rc.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_recon(ref)), "tests/golden/ref_recon.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- everywhere

@pytest.mark.parametrize("name", rc.picture_names())
def test_command_lists_are_well_formed(name):
    pic = rc.picture(name)
    d = rc.derive(pic)
    assert rc.well_formed(pic, d) is None, rc.well_formed(pic, d)
    assert len(d.order)
    if any(pcs.waits_for(d.ctus, pic.ncx, rs) for rs in d.order):
        assert rc.order_defect(d.ctus, pic.ncx, pic.ncy, d.order[::-1]) is not None, "the restated order check accepts a reversed order"
    for s in d.specs:                                   # what the record passes' contracts ask of a record
        assert d.off_of[s["rid"]] % 4 == 0 and (1 << (s["lw"] + s["lh"])) >= 4 and s["lw"] <= 6 and s["lh"] <= 6
        if s.get("ts"):
            assert 1 <= s["lw"] <= 5 and 1 <= s["lh"] <= 5 and s["lw"] + s["lh"] >= 3
    for s, first in ((d.inter, d.bin_first), (d.skip, d.ts_first)):
        assert first[0][0] == 0 and first[0][-1] == first[1][0] and first[1][-1] == len(s)


@pytest.mark.parametrize("name", rc.picture_names())
def test_oracle_reproduces_reference_digests(golden, orc, ref, name):
    assert name in golden, f"{name} is not in ref_recon.json: regenerate it (tests/golden/README.md)"
    got = rc.oracle_digests(orc, name)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle side's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the first sample")


def test_no_picture_left_out(golden):
    assert list(golden) == rc.picture_names()


def test_premises_of_the_listed_pictures():
    total = Counter()
    for name in rc.picture_names():
        pic = rc.picture(name)
        assert pic.width <= 264 and pic.height <= 136
        total.update(rc.census(pic, rc.derive(pic)))
    missing = [p for p in rc.PREMISES if not total[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"


def test_generator_stays_inside_the_dequant_limits():
    """qp + dep_quant <= 75 and |level| * scale * 16 + bd_offset < 2^31 on every coded block (for BDPCM: of the accumulated level)."""
    for name in rc.picture_names():
        pic = rc.picture(name)
        d = rc.derive(pic)
        for s in d.specs:
            tsf = bool(s.get("ts"))
            dep = 0 if tsf else s["dep"]
            assert s["qp"] + dep <= 75
            c = s["c"].astype(np.int64)
            if tsf and s["bdpcm"]:
                c = np.cumsum(c, axis=0 if s["vert"] else 1)
            assert np.abs(c).max() <= rc._level_limit(pic, s["lw"], s["lh"], s["qp"], dep, tsf)

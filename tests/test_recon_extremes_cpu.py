"""The directed worst-case pictures of tests/recon_extreme_cases.py, CPU side: premises first, then the pin.

* Premises, counted before anything is compared: from int64 restatements (dequantisation, both transform stages and the inverse LFNST's
  sums of every block; the residual add of every block in its five forms) and from the oracle side's run — first-stage sums beyond the
  transform range before the clip, residuals on their bound, levels at the ends of the packed stream and beyond int16, packed beside int32
  records in one workgroup's worth of records, overshoot at both ends in every add form (batched epilogues and RESID commands, widths 1 and
  2), both ends of the bin search and of chroma_scale_coeff, every picture's reconstruction clipping at both ends, the tools and shapes of the
  intra-predictor class, and — from the oracle's predictors run once more with headroom — cubic filter, PDPC and MIP outputs below 0 and
  above the maximum before their clip.  Every restated residual must equal the oracle's.  What the domain does not hold is named
  (recon_extreme_cases.UNREACHABLE, with its reason).  CCLM's diff = 0 branch, a = +15 / -15 and outputs beyond the range before the clip
  are counted inside the oracle's own run, per chroma format and `collocated`; luma inside the LMCS slices holds both ends of the range.
* The generator stays inside the dequant limits, and the shim refuses no listed picture (a refusal fails, nothing skips on it).
* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): oracle side == the reference, planes whole and cached chroma scales.
* Everywhere: the oracle side reproduces tests/golden/ref_recon_extremes.json, no picture is left out, the command lists are well-formed
  (the GPU test launches only such lists), and the sensitivity table of recon_extreme_cases is recomputed against the digests: each
  narrowing, applied to the oracle side's Python glue alone, changes the listed pictures the table names and the pictures of T0-T9 it names."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

import picture_cases as pcs
import recon_extreme_cases as xc
import ref_lib
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
    return xc.load_golden()


@pytest.fixture(scope="module")
def sides(orc):
    """name -> (derived inputs, the oracle side's planes, scale table, arena): computed once, nobody writes to them."""
    out = {}
    for name in xc.picture_names():
        d = rc.derive(xc.picture(name))
        out[name] = (d,) + tuple(rc.oracle_side(orc, d))
    return out


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


# ---------------------------------------------------------------------------------------------------------------- premises

def test_the_list_spreads_over_bit_depths_formats_and_ctu_sizes():
    pics = [xc.picture(n) for n in xc.picture_names()]
    assert 10 <= len(pics) <= 14
    assert all(p.width <= 264 and p.height <= 136 for p in pics)
    assert {p.bd for p in pics} == {8, 10, 12} and {p.idc for p in pics} == {0, 1, 2, 3} and {p.ctb_log2 for p in pics} == {5, 6, 7}
    assert any(p.rbits == 18 for p in pics), "no picture at transform range 18"
    assert any(all(cu["tree_type"] != 0 for ctu in p.ctus for cu in ctu) for p in pics), "no dual-tree picture"
    assert any(not p.chroma_scale_flag for p in pics) and any(len({s[1] for s in p.slices}) == 2 for p in pics), "slices with and without LMCS"
    for p in pics:                                      # the starting planes hold the ends of the range only
        for plane in p.planes[:3 if p.idc else 1]:
            assert set(np.unique(plane).tolist()) <= {0, (1 << p.bd) - 1}
    assert all(n in xc.picture_names() for n in xc.OLD_PATH + xc.RASTER_TOO + xc.UNPACKED_TOO + xc.PREDICTOR_PICTURES)


def test_premises_of_the_transform_and_residual_classes(orc, sides):
    total = Counter()
    for name in xc.picture_names():
        d, planes, _table, arena = sides[name]
        n = xc.census(orc, d.pic, d, planes, arena)
        assert n["reconstruction clips at 0"] > 0 and n["reconstruction clips at the maximum"] > 0, f"{name}: its reconstruction does not clip at both ends"
        total.update(n)
    missing = [p for p in xc.PREMISES if not total[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"
    print("\n".join(f"{total[p]:7d}  {p}" for p in xc.PREMISES))


def test_premises_of_the_predictor_class(orc, sides):
    units, near, over = Counter(), Counter(), Counter()
    for name in xc.picture_names():
        d, planes, _table, _arena = sides[name]
        units.update(xc.unit_census(d.pic))
        n = xc.predictor_overshoot_census(orc, d.pic, d, planes)          # asserts that no convex predictor leaves the range
        over.update(n)
        if name in xc.PREDICTOR_PICTURES:
            near.update(xc.neighbour_census(d.pic, d, planes))
            if d.pic.bd != 12:
                assert n["cubic filter: samples below 0 before the clip"] and n["cubic filter: samples above the maximum before the clip"], name
    missing = [p for p in xc.UNIT_PREMISES if not units[p]] + [p for p in xc.NEIGHBOUR_PREMISES if not near[p]] + [p for p in xc.OVERSHOOT_PREMISES if not over[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"
    print("\n".join(f"{over[p]:7d}  {p}" for p in sorted(over)))


def test_what_the_domain_does_not_hold():
    """recon_extreme_cases.UNREACHABLE names the two classes with their reasons; the reasons are facts of the kernel's and the reference's code
    (cited there), not something a restatement can show, so nothing is recomputed here."""
    assert len(xc.UNREACHABLE) == 2 and all(len(why) > 80 for why in xc.UNREACHABLE.values())


def test_premises_of_cclm_and_inverse_lmcs(orc, sides):
    """CCLM from the oracle's own run (orc_cclm_debug_stats): per chroma format and `collocated` value the diff = 0 branch, a = +15 and -15
    (the ends of what the derivation gives), outputs below 0 and above the maximum before the clip.  Inverse LMCS: the reconstructed luma
    inside the slices that use LMCS holds 0 and the maximum, in every picture with such a slice."""
    total = Counter()
    with_lmcs = 0
    for name in xc.picture_names():
        d, planes, _table, _arena = sides[name]
        pic = d.pic
        total.update(xc.cclm_census(orc, pic, d))
        used = np.array([sl[1] for sl in pic.slices], np.uint8)
        mask = pcs.lmcs_mask(pic.width, pic.height, pic.ctb_log2, pic.slice_idx, used)
        if mask.any():
            with_lmcs += 1
            inside = planes[0][mask]
            assert (inside == 0).any() and (inside == (1 << pic.bd) - 1).any(), f"{name}: luma inside its LMCS slices misses an end of the range"
            lut = xc.inverse_lut(pic)
            assert lut[0] != 0 and lut[-1] != 0, "the inverse table moves the lower end"
    assert with_lmcs >= 6
    missing = [p for p in xc.CCLM_PREMISES if not total[p]]
    assert not missing, f"the listed pictures do not reach: {missing}"
    print("\n".join(f"{total[p]:7d}  {p}" for p in sorted(total)))


def test_generator_stays_inside_the_dequant_limits():
    """qp + dep_quant <= 75 and |level| * scale * 16 + bd_offset < 2^31 on every coded block (for BDPCM: of the accumulated level)."""
    for name in xc.picture_names():
        pic = xc.picture(name)
        d = rc.derive(pic)
        for s in d.specs:
            tsf = bool(s.get("ts"))
            dep = 0 if tsf else s["dep"]
            assert s["qp"] + dep <= 75
            c = s["c"].astype(np.int64)
            if tsf and s["bdpcm"]:
                c = np.cumsum(c, axis=0 if s["vert"] else 1)
            assert np.abs(c).max() <= rc._level_limit(pic, s["lw"], s["lh"], s["qp"], dep, tsf)


@pytest.mark.parametrize("name", xc.picture_names())
def test_command_lists_are_well_formed(name):
    pic = xc.picture(name)
    d = rc.derive(pic)
    assert rc.well_formed(pic, d) is None, rc.well_formed(pic, d)
    assert len(d.order)
    if any(pcs.waits_for(d.ctus, pic.ncx, rs) for rs in d.order):
        assert rc.order_defect(d.ctus, pic.ncx, pic.ncy, d.order[::-1]) is not None
    for s in d.specs:
        assert d.off_of[s["rid"]] % 4 == 0 and (1 << (s["lw"] + s["lh"])) >= 4 and s["lw"] <= 6 and s["lh"] <= 6
        if s.get("ts"):
            assert 1 <= s["lw"] <= 5 and 1 <= s["lh"] <= 5 and s["lw"] + s["lh"] >= 3


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", xc.picture_names())
def test_live_reconstruction_equals_the_reference(ref, sides, name):
    _need(ref)
    d, got, table, _arena = sides[name]
    pic = d.pic
    ret, want, scales, twice = rc.run_reference(ref, pic)
    assert ret == 0, f"{name}: the shim refused the picture ({ret}): the list left the domain"
    assert not twice, f"{name}: the reference cached two different scales for the units at {twice[:4]}"
    diff = rc.first_difference(want, got)
    assert diff is None, f"{name}: reference / oracle side: {diff}"
    assert any(np.any(w != p) for w, p in zip(want, pic.planes))
    if table is not None:
        t = table.reshape(d.tpic.uy, d.tpic.ux)
        for (ux, uy) in d.routed:
            key = (ux * pic.size_y, uy * pic.size_y)
            assert key in scales, f"{name}: the host routes unit {key} to the TB passes, the reference never asked for its scale"
            assert scales[key] == t[uy, ux], f"{name}: unit {key}: the reference cached {scales[key]}, orc_lmcs_vpdu_scale_pass gives {t[uy, ux]}"
    else:
        assert not scales and not d.routed


def test_live_shim_refuses_no_listed_picture(ref):
    _need(ref)
    refused = [n for n in xc.picture_names() if rc.run_reference(ref, xc.picture(n))[0] != 0]
    assert not refused, f"the shim refused {refused}: a failure of the list, not a reason to skip"


def test_live_fixture_is_fresh(ref):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(xc.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_recon_extremes(ref)), \
            "tests/golden/ref_recon_extremes.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- everywhere

@pytest.mark.parametrize("name", xc.picture_names())
def test_oracle_reproduces_reference_digests(golden, sides, ref, name):
    assert name in golden, f"{name} is not in ref_recon_extremes.json: regenerate it (tests/golden/README.md)"
    d, planes, table, _arena = sides[name]
    got = rc.digests(d.pic, d, planes, table)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle side's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the first sample")


def test_no_picture_left_out(golden):
    assert list(golden) == xc.picture_names()


def _planes_differ(rec, pic, planes):
    return any(rc.sha(planes[c]) != rec[f"p{c}"] for c in range(3 if pic.idc else 1))


@pytest.mark.parametrize("narrowing", xc.NARROWINGS)
def test_sensitivity(orc, golden, narrowing):
    """The narrowing changes exactly the pictures the table names — of this list (and at least one), and of T0-T9."""
    quiet = rc.load_golden()
    here = [n for n in xc.picture_names() if _planes_differ(golden[n], xc.picture(n), xc.narrowed_oracle_side(orc, rc.derive(xc.picture(n)), narrowing))]
    there = [n for n in rc.picture_names() if _planes_differ(quiet[n], rc.picture(n), xc.narrowed_oracle_side(orc, rc.derive(rc.picture(n)), narrowing))]
    assert here, f"no listed picture notices '{narrowing}'"
    assert (here, there) == xc.SENSITIVITY[narrowing], f"'{narrowing}' is noticed by {here} and {there}: recon_extreme_cases.SENSITIVITY says {xc.SENSITIVITY[narrowing]}"
    # the narrowing is gone again: the plain oracle side still hashes to the fixture
    name = here[0]
    d = rc.derive(xc.picture(name))
    assert not _planes_differ(golden[name], d.pic, rc.oracle_side(orc, d)[0])


def test_packed_stream_of_the_list_round_trips():
    """levels_cases.pack_all on the list's levels: the int16 ends survive the packed stream, the blocks beyond int16 are flagged int32."""
    import levels_cases as lc
    for name in xc.picture_names():
        d = rc.derive(xc.picture(name))
        blocks = [s["c"] for s in d.specs]
        stream, lv = lc.pack_all(blocks)
        for c, r in zip(blocks, lv):
            wide = bool(r["flags"] & abi.LEVELS_INT32)
            assert wide == bool(c.max() > 32767 or c.min() < -32768)
            if not wide:
                h, w = c.shape
                assert np.array_equal(lc.unpack(int(r["groups"]), stream, int(r["first"]), w, h), c)


@pytest.mark.parametrize("name", xc.picture_names())
def test_recorder_gives_the_derived_inputs(name):
    """The recorder (ffvvc_amd/host/recorder.c, host code) on the list: its commands, records, side records, packed level stream and arena
    equal derive()'s, which the GPU test uploads, with packing on and off — levels of +32767 / -32768 in the stream, blocks beyond int16 flagged
    int32 (tests/test_recorder_cpu.py's comparison on this content)."""
    import recorder_cases as rk
    lib = abi.load()
    pic = xc.picture(name)
    d = rc.derive(pic)
    p = rk.pods(pic)
    for pack in (True, False):
        o = rk.record(lib, pic, pack, p=p)
        bad = rk.differences(lib, pic, d, o, pack)
        assert not bad, f"{name}, packing {'on' if pack else 'off'}: {bad} differ from derive()"
        assert pcs.order_check(lib, o.ctus, pic.ncx, pic.ncy, o.order) == 0 and rc.order_defect(o.ctus, pic.ncx, pic.ncy, o.order) is None
        if pack:
            wide = (o.lv["flags"] & abi.LEVELS_INT32) != 0
            assert wide.any() and not wide.all(), "the recorder's stream holds packed and int32 blocks"
            assert (o.levels == 32767).any() and (o.levels == -32768).any(), "the ends of int16 in the recorder's stream"

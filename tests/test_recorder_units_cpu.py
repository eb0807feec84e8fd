"""CPU: the recorder's unit entry (vvc355_rec_ctu_units / vvc355_rec_units, include/vvc_mi355_rec.h) held to recorder_units_cases' numpy.

  1. layouts, sizes and codes are the header's (the C compiler's offsetof against the ctypes mirrors);
  2. the premises: what the listed pictures must contain, counted from the unit descriptions before anything is compared;
  3. every listed picture and 32 sweep pictures: commands, CTU table, order, the three TB lists with side records, level stream and arena
     (recorder_cases.differences on the extended derive(), packing on and off), the vvc355_ciip_cu / inter / affine / GPM lists and the
     ctu_first tables byte for byte, the cu / tu records with their sidecars and the motion records as sets per CTU and through the tables
     they paint;
  4. CTUs fed in reverse and in a seeded shuffle give the same result (late_keep aside);
  5. without CIIP units, vvc355_rec_ctu_units gives the vvc355_rec_result vvc355_rec_ctu gives, byte for byte;
  6. every new refusal returns its code, and the same object then records a good picture like a fresh one; vvc355_rec_ctu still refuses a
     CIIP unit with VVC355_REC_E_CIIP;
  7. tools/recorder_units_check.c with recorder.c and levels_pack.c under -fsanitize=address,undefined, stand-alone, on three pictures.
"""
import ctypes
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import mvf_unit_cases as mu
import picture_cases as pcs
import recorder_cases as rk
import recorder_units_cases as uc
import ref_recon_cases as rc
from conftest import ROOT
from ffvvc_amd import abi
from test_picture_cpu import _enum

HEADER = os.path.join(ROOT, "include", "vvc_mi355_rec.h")
SWEEP = 32
MIRRORS = (("vvc355_rec_pu", abi.RecPu, 32), ("vvc355_rec_units_result", abi.RecUnitsResult, 144), ("vvc355_rec_cu", abi.RecCu, 56),
           ("vvc355_rec_result", abi.RecResult, 416), ("vvc355_rec_params", abi.RecParams, 48), ("vvc355_rec_deblock_tus", abi.RecDeblockTus, 32))
CODES = ("ARGS", "MIXED", "CIIP_SHAPE", "MOTION", "COUNT")


@pytest.fixture(scope="module")
def lib():
    return abi.load()


_derived = {}


def listed(name):
    """(picture, derive(picture)) of a listed picture, made once and left unchanged."""
    if name not in _derived:
        pic = uc.picture(name)
        _derived[name] = (pic, uc.derive(pic))
    return _derived[name]


# ---------------------------------------------------------------------------------------------------------------- 1

def test_layouts_and_codes_match_the_header(tmp_path):
    text = open(HEADER).read()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vvc_mi355_rec.h"', "int main(void) {"]
    for cname, cls, size in MIRRORS:
        assert ctypes.sizeof(cls) == size, cname
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{n} %zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for cname, cls, size in MIRRORS:
        assert int(got[cname]) == size, cname
        for n, _ in cls._fields_:
            assert int(got[f"{cname}.{n}"]) == getattr(cls, n).offset, (cname, n)
    assert re.search(r"32 bytes, no\s+\*?\s*implicit padding", text)
    codes = _enum(text, "VVC355_RECU_E_")
    assert len(codes) == len(CODES)
    for i, n in enumerate(CODES):
        assert codes["VVC355_RECU_E_" + n] == getattr(abi, "RECU_E_" + n) == -(21 + i), n
    assert not set(codes.values()) & set(_enum(text, "VVC355_REC_E_").values())
    assert abi.BATCH_SIGNATURES["rec_ctu_units"] == ("i", "piiippi") and abi.BATCH_SIGNATURES["rec_units"] == ("i", "pp")
    out_of_scope = text[text.index("Out of scope here"):text.index("Threads:")]
    assert "scaling lists" in out_of_scope and "ACT" in out_of_scope
    assert "CIIP" not in out_of_scope and "cu_rec" not in out_of_scope and "motion" not in out_of_scope


# ---------------------------------------------------------------------------------------------------------------- 2

def test_the_listed_pictures_hold_the_premises(lib):
    total = Counter()
    for name in uc.picture_names():
        pic, d = listed(name)
        assert pic.width <= 264 and pic.height <= 136
        total.update(uc.census(pic, d))
    missing = [p for p in uc.PREMISES if not total[p]]
    assert not missing, f"no listed picture has: {missing}"
    # a CTU of 128 without an intra unit whose CIIP unit is recorded AFTER the scaled chroma blocks it keeps in the walk
    pic, d = listed("UD")
    o = uc.record(lib, pic)
    assert pic.ctb_log2 == 7 and not any(cu["pred_mode"] == 1 for cu in pic.ctus[0]) and pic.ctus[0][-1]["ciip_flag"]
    assert o.late_keep == 2 and o.stats["walk_scaled"] == 2 and d.stats["walk_scaled"] == 2
    # ... and pictures where it is a neighbour CTU's CIIP unit that keeps them
    assert sum(uc.record(lib, listed(n)[0]).stats["walk_scaled"] for n in ("U5", "U8")) > 0


# ---------------------------------------------------------------------------------------------------------------- 3

def _check_equal(lib, pic, d):
    p = uc.pods(pic)
    for pack in (True, False):
        o = uc.record(lib, pic, pack, p=p)
        bad = rk.differences(lib, pic, d, o, pack) + uc.unit_differences(pic, d, o)
        assert not bad, f"{pic.name}, packing {'on' if pack else 'off'}: {bad} differ from the expectation"
        assert not o.cmds["pad_"].any(), "pad bytes of the commands"
        ciip = o.cmds[o.cmds["kind"] == abi.RECON_CIIP]
        assert not ciip["resid"].any() and not ciip["joint"].any(), "resid / joint of the CIIP commands go up as 0"
        assert pcs.order_check(lib, o.ctus, pic.ncx, pic.ncy, o.order) == 0
        assert rc.order_defect(o.ctus, pic.ncx, pic.ncy, o.order) is None
        # every block of a CIIP unit: KEEP, no joint bits in the record, a RESID command
        n_i = len(d.intra)
        for s, r in zip(d.specs[n_i:], np.concatenate([o.inter.view(np.uint8).reshape(-1, 16), o.ts.view(np.uint8).reshape(-1, 16)])):
            if s["ciip"]:
                rec = r.view(rk.INTER if "tu_flags" in s else rk.TS)[0]
                assert rec["flags"] & 8 and not (rec["joint_mts"] & 15 if "tu_flags" in s else rec["joint"]), (pic.name, s["rid"])
    return o


@pytest.mark.parametrize("name", uc.picture_names())
def test_listed_pictures_equal_the_expectation(lib, name):
    pic, d = listed(name)
    o = _check_equal(lib, pic, d)
    u = o.u
    # the CIIP records name CIIP commands of their own unit and component
    for r in u.ciip:
        for c in range(3):
            if r["cmd"][c] != uc.NO_CMD:
                cmd = o.cmds[int(r["cmd"][c])]
                assert (cmd["kind"], cmd["c_idx"], cmd["x0"], cmd["y0"], cmd["w"], cmd["h"]) == (abi.RECON_CIIP, c, r["x0"], r["y0"], r["cb_width"], r["cb_height"])
    assert len(u.ciip) == sum(cu["ciip_flag"] for ctu in pic.ctus for cu in ctu)
    # a CTU with a CIIP unit keeps its list and is not LIGHT
    for rs, ctu in enumerate(pic.ctus):
        if any(cu["ciip_flag"] for cu in ctu):
            assert o.ctus[rs]["n_cmd"] and not o.ctus[rs]["flags"] & abi.RECON_CTU_LIGHT


@pytest.mark.parametrize("k0", range(0, SWEEP, 8))
def test_sweep_pictures_equal_the_expectation(lib, k0):
    for k in range(k0, k0 + 8):
        pic = uc.sweep_picture(k)
        _check_equal(lib, pic, uc.derive(pic))


def test_the_comparison_sees_a_wrong_rule(lib):
    """Sensitivity of the byte comparisons: the expectation without the CIIP rules differs from the recorder on a picture with CIIP units."""
    pic, d = listed("U5")
    o = uc.record(lib, pic)
    plain = rc.derive(pic)                                       # CIIP units taken for ordinary inter units
    assert rk.differences(lib, pic, plain, o, True)
    e = uc.expect_units(pic, d)
    assert len(e.ciip) > 10 and len(e.affine) > 2 and len(e.gpm) > 2 and len(e.inter) > 10
    o.u.ciip["scratch_off"][-1] += 1
    assert "ciip" in uc.unit_differences(pic, d, o)


# ---------------------------------------------------------------------------------------------------------------- 4

def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("cmds", "ctus", "order", "intra", "inter", "ts", "lv", "levels", "arena")) and \
        a.head == b.head


def _same_units(a, b):
    return all(getattr(a.u, k).tobytes() == getattr(b.u, k).tobytes() for k in uc.LISTS) and a.u.totals == b.u.totals


@pytest.mark.parametrize("name", ["U1", "U2", "U5", "U8"])
def test_ctus_in_any_order_give_the_same_result(lib, name):
    pic, _d = listed(name)
    p = uc.pods(pic)
    n = len(pic.ctus)
    raster = uc.record(lib, pic, True, p=p)
    for order in (np.arange(n)[::-1], np.random.default_rng(0x0DE2).permutation(n)):
        other = uc.record(lib, pic, True, order=order, p=p)
        assert _same(raster, other) and _same_units(raster, other), name


# ---------------------------------------------------------------------------------------------------------------- 5

@pytest.mark.parametrize("name", ["T0", "T2", "T5"])
def test_without_ciip_units_both_entries_give_the_same_result(lib, name):
    k = list(rc._LISTED).index(name)
    pic = uc.dress(rc.draw(name, rc.SEED + k, **rc._LISTED[name]), k, 0.0)
    assert not any(cu["ciip_flag"] for ctu in pic.ctus for cu in ctu)
    p = uc.pods(pic)
    assert name != "T0" or not any(p.has_inter)                   # all intra: every call has null pus
    for pack in (True, False):
        a, b = rk.record(lib, pic, pack, p=p), uc.record(lib, pic, pack, p=p)
        assert _same(a, b) and a.late_keep == b.late_keep and bytes(a.res)[abi.RecResult.n_levels.offset:] == bytes(b.res)[abi.RecResult.n_levels.offset:]


# ---------------------------------------------------------------------------------------------------------------- 6

def test_refusals_leave_the_recorder_usable(lib):
    pic, d = listed("U5")
    fresh = uc.record(lib, pic)
    units = [cu for ctu in pic.ctus for cu in ctu]
    first_of = {k: next(i for i, cu in enumerate(units) if "pu" in cu and cu["pu"]["kind"] == k and not cu["ciip_flag"] and cu["pu"]["nsx"] == 1)
                for k in (mu.PLAIN, mu.AFFINE, mu.GPM)}
    sub = next(i for i, cu in enumerate(units) if "pu" in cu and cu["pu"]["nsx"] * cu["pu"]["nsy"] > 1)
    ciip = next(i for i, cu in enumerate(units) if cu["ciip_flag"])
    plain = first_of[mu.PLAIN]
    rs_of = np.searchsorted(rk.pods(pic).first, np.arange(len(units)), side="right") - 1

    def setf(arr, i, field, value):
        def change(p):
            getattr(p, arr)[field][i] = value
        return change

    def gpm_pred(p):                                              # pred_flag of the first part -> 3
        p.motion[int(p.motion_off[first_of[mu.GPM]]) + 5] = 3

    def small_ciip(p):
        p.cus["w"][ciip], p.cus["h"][ciip] = 4, 8

    cases = [
        (abi.RECU_E_ARGS, setf("pus", plain, "motion", 0), "an inter unit without motion"),
        (abi.RECU_E_CIIP_SHAPE, small_ciip, "a CIIP unit of 32 samples"),
        (abi.RECU_E_CIIP_SHAPE, setf("cus", ciip, "pred_mode", 2), "a CIIP unit that is not an inter unit"),
        (abi.RECU_E_CIIP_SHAPE, setf("pus", ciip, "kind", mu.GPM), "a CIIP unit with GPM motion"),
        (abi.RECU_E_CIIP_SHAPE, setf("pus", ciip, "num_sb_x", 2), "a CIIP unit with a sub-block grid"),
        (abi.RECU_E_CIIP_SHAPE, setf("cus", ciip, "tree_type", 2), "a CIIP unit on the chroma tree"),
        (abi.RECU_E_CIIP_SHAPE, setf("cus", ciip, "tree_type", 1), "a CIIP unit on the dual-tree luma tree"),
        (abi.RECU_E_MOTION, setf("pus", plain, "kind", 3), "kind above GPM"),
        (abi.RECU_E_MOTION, setf("pus", sub, "num_sb_x", 3), "a sub-block grid that does not divide the unit"),
        (abi.RECU_E_MOTION, setf("pus", plain, "num_sb_y", 0), "an empty sub-block grid"),
        (abi.RECU_E_MOTION, setf("pus", first_of[mu.AFFINE], "motion_model_idc", 3), "an affine model of 3"),
        (abi.RECU_E_MOTION, setf("pus", first_of[mu.AFFINE], "pred_flag", 0), "an affine unit without a list"),
        (abi.RECU_E_MOTION, setf("pus", first_of[mu.GPM], "gpm_partition_idx", 64), "partition 64"),
        (abi.RECU_E_MOTION, gpm_pred, "a GPM part predicted from both lists"),
    ]
    small_affine = next((i for i, cu in enumerate(units) if cu["w"] == 4 and "pu" in cu and not cu["ciip_flag"]), None)
    if small_affine is not None:
        cases.append((abi.RECU_E_MOTION, lambda p: (setf("pus", small_affine, "kind", mu.AFFINE)(p), setf("pus", small_affine, "pred_flag", 1)(p),
                                                    setf("pus", small_affine, "motion_model_idc", 1)(p)), "an affine unit 4 wide"))
    rec = lib.vvc355_rec_create()
    try:
        res, ures = abi.RecResult(), abi.RecUnitsResult()
        assert lib.vvc355_rec_ctu_units(rec, 0, 0, 0, None, None, 0) == abi.REC_E_STATE          # no picture begun
        assert lib.vvc355_rec_units(rec, ctypes.byref(ures)) == abi.REC_E_STATE
        assert lib.vvc355_rec_deblock_units(rec, ctypes.byref(abi.RecDeblockTus())) == abi.REC_E_STATE
        assert lib.vvc355_rec_ctu_units(None, 0, 0, 0, None, None, 0) == abi.REC_E_ARGS
        par = rk.params(pic)

        def good_again(what):
            """The recorder is where begin_picture left it: the picture goes through the same object without another begin."""
            p = uc.pods(pic)
            assert uc.feed(lib, rec, pic, p) == 0, what
            assert lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
            o = rk.snapshot(lib, rec, res)
            o.u = uc.units_snapshot(lib, rec, len(pic.ctus))
            assert _same(fresh, o) and _same_units(fresh, o), what

        for want, change, what in cases:
            p = uc.pods(pic)
            change(p)
            assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
            assert uc.feed(lib, rec, pic, p) == want, what
            good_again(what)
        # an inter unit in a CTU given without pus
        p = uc.pods(pic)
        rs = int(rs_of[plain])
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        assert lib.vvc355_rec_ctu_units(rec, rs, 0, 0, p.cus.ctypes.data + rk.CU.itemsize * int(p.first[rs]), None, int(p.first[rs + 1] - p.first[rs])) == abi.RECU_E_ARGS
        good_again("null pus")
        # a slice index that does not fit the records' byte
        for bad_slice in (-1, 256):
            assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
            assert lib.vvc355_rec_ctu_units(rec, 0, 0, 255, p.cus.ctypes.data, p.pus.ctypes.data, int(p.first[1])) == 0
            assert lib.vvc355_rec_ctu_units(rec, 1, 0, bad_slice, p.cus.ctypes.data + rk.CU.itemsize * int(p.first[1]),
                                            p.pus.ctypes.data + uc.PU.itemsize * int(p.first[1]), int(p.first[2] - p.first[1])) == abi.RECU_E_ARGS
            good_again("slice out of range")
        # many CIIP units on the chroma tree, which make commands and no vvc355_ciip_cu: refused, not recorded
        many = np.zeros(300, rk.CU)
        many["w"], many["h"], many["tree_type"], many["ciip_flag"] = 8, 8, 2, 1
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        assert lib.vvc355_rec_ctu_units(rec, 0, 0, 0, many.ctypes.data, None, 300) == abi.RECU_E_CIIP_SHAPE
        good_again("chroma-tree CIIP units")
        # a CIIP unit with a side above 64 (CTU 128)
        wide_pic, _wd = listed("U2")
        wide_units = [cu for ctu in wide_pic.ctus for cu in ctu]
        wide = next(i for i, cu in enumerate(wide_units) if cu["pred_mode"] == 0 and max(cu["w"], cu["h"]) == 128)
        w = uc.pods(wide_pic)
        w.cus["ciip_flag"][wide] = 1
        wide_par = rk.params(wide_pic)
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(wide_par)) == 0
        assert uc.feed(lib, rec, wide_pic, w) == abi.RECU_E_CIIP_SHAPE
        w = uc.pods(wide_pic)
        assert uc.feed(lib, rec, wide_pic, w) == 0 and lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        good_again("a CIIP unit 128 wide")
        # the two entries in one picture, either way round
        plain_pic = rc.picture("T5")
        q = rk.pods(plain_pic)
        for units_first in (False, True):
            assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
            calls = [lambda: lib.vvc355_rec_ctu(rec, 0, 0, q.cus.ctypes.data, int(q.first[1])),
                     lambda: lib.vvc355_rec_ctu_units(rec, 1, 0, 0, p.cus.ctypes.data + rk.CU.itemsize * int(p.first[1]),
                                                      p.pus.ctypes.data + uc.PU.itemsize * int(p.first[1]), int(p.first[2] - p.first[1]))]
            if units_first:
                calls.reverse()
            assert calls[0]() == 0 and calls[1]() == abi.RECU_E_MIXED
            good_again("mixed entries")
        # vvc355_rec_units after a picture of vvc355_rec_ctu; a null result
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(rk.params(plain_pic))) == 0
        assert rk.feed(lib, rec, plain_pic, q) == 0 and lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
        assert lib.vvc355_rec_units(rec, ctypes.byref(ures)) == abi.RECU_E_MIXED
        assert lib.vvc355_rec_units(rec, None) == abi.RECU_E_ARGS
        assert lib.vvc355_rec_deblock_units(rec, ctypes.byref(abi.RecDeblockTus())) == abi.RECU_E_MIXED and lib.vvc355_rec_deblock_units(rec, None) == abi.RECU_E_ARGS
        # more than 65535 records of a kind in one CTU: 65536 times the same 8x8 intra unit
        one = np.zeros(65536, rk.CU)
        one["w"], one["h"], one["pred_mode"] = 8, 8, 1
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        assert lib.vvc355_rec_ctu_units(rec, 0, 0, 0, one.ctypes.data, None, 65536) == abi.RECU_E_COUNT
        assert lib.vvc355_rec_ctu_units(rec, 0, 0, 0, one.ctypes.data, None, 65535) == 0
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        good_again("count")
    finally:
        lib.vvc355_rec_destroy(rec)
    assert not rk.differences(lib, pic, d, fresh, True)


def test_rec_ctu_still_refuses_ciip_units(lib):
    pic, _d = listed("U5")
    p = uc.pods(pic)
    rec = lib.vvc355_rec_create()
    try:
        par = rk.params(pic)
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        assert rk.feed(lib, rec, pic, p) == abi.REC_E_CIIP
    finally:
        lib.vvc355_rec_destroy(rec)


# ---------------------------------------------------------------------------------------------------------------- 7

# the runtimes linked in: the program then runs the same whatever else a machine loads into its processes
SAN_FLAGS = ["-std=c11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recorder_units_check")
    one = tmp / "one.c"
    one.write_text("int main(void) { return 0; }\n")
    flags = SAN_FLAGS
    if subprocess.run(["gcc", *flags, str(one), "-o", str(tmp / "one")], capture_output=True).returncode:
        flags = SAN_FLAGS[:-2]                                  # no static runtimes installed: the shared ones
        if subprocess.run(["gcc", *flags, str(one), "-o", str(tmp / "one")], capture_output=True).returncode:
            pytest.skip("gcc cannot build a one-line program with -fsanitize=address,undefined here")
    exe = tmp / "recorder_units_check"
    srcs = [os.path.join(ROOT, "tools", "recorder_units_check.c"), os.path.join(ROOT, "ffvvc_amd", "host", "recorder.c"),
            os.path.join(ROOT, "ffvvc_amd", "host", "levels_pack.c")]
    subprocess.check_call(["gcc", *flags, "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), *srcs, "-o", str(exe)])
    return exe, tmp


@pytest.mark.parametrize("name", ["U1", "U2", "U5"])          # 4:4:4 with tiles, CTU 32; 4:2:2 at CTU 128; 4:2:0 with units down to 4 wide
def test_stand_alone_run_is_clean_under_the_sanitizers(lib, check_program, name):
    exe, tmp = check_program
    pic, _d = listed(name)
    path = tmp / f"{name}.dump"
    uc.dump(pic, path)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    want = "%016x" % uc.digest(uc.record(lib, pic, True))
    assert r.stdout.split() == [want, want], f"{name}: the stand-alone runs print {r.stdout.split()}, the library's run {want}"

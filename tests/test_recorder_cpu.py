"""CPU: the recorder (include/vvc_mi355_rec.h, ffvvc_amd/host/recorder.c) held byte for byte to ref_recon_cases.derive(), the numpy
restatement of INTEGRATION.md section 3 whose outputs tests/test_ref_recon_cpu.py holds to the reference's digests.

  1. layouts, sizes and codes are the header's (the C compiler's offsetof against the ctypes mirrors);
  2. every listed picture and 48 sweep pictures: commands (pad bytes zero), CTU table, order, n_work, the three grouped lists with their
     first-tables, side records and level stream, the arena after fill_arena, the statistics — with packing on and off
     (recorder_cases.differences: the arena-slot numbering and the RESID commands' `resid` are normalised, nothing else);
  3. vvc355_recon_order_check accepts every order;
  4. sensitivity: each misreading of ref_recon_cases.MISREADINGS applied to derive() makes the comparison fail on every picture the
     module's table lists for it;
  5. CTUs fed in reverse and in a seeded shuffle give the same result (late_keep aside: it counts what the order of the calls decides);
  6. deferred KEEP: a directed picture — CTU 128, an inter unit with coded chroma in the 64x64 unit at x = 64, an intra unit later in the
     same CTU — whose two chroma blocks are decided by a unit recorded after them; without the intra unit they go to the batched pass;
  7. every refusal kind returns its code, and the same object then records a good picture like a fresh one;
  8. tools/recorder_check.c with recorder.c and levels_pack.c under -fsanitize=address,undefined, stand-alone, on three pictures.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import picture_cases as pcs
import recorder_cases as rk
import ref_recon_cases as rc
from conftest import ROOT
from ffvvc_amd import abi
from test_picture_cpu import _enum

HEADER = os.path.join(ROOT, "include", "vvc_mi355_rec.h")
SWEEP = 48
MIRRORS = (("vvc355_rec_tb", abi.RecTb, 32), ("vvc355_rec_tu", abi.RecTu, 32), ("vvc355_rec_cu", abi.RecCu, 56),
           ("vvc355_rec_params", abi.RecParams, 48), ("vvc355_rec_result", abi.RecResult, 416))
CODES = ("ARGS", "STATE", "PARAMS", "CTU_RANGE", "CTU_TWICE", "CU_RECT", "TB_RECT", "SIDE", "C_IDX", "LEVELS", "CIIP", "NOMEM")


@pytest.fixture(scope="module")
def lib():
    return abi.load()


_derived = {}


def listed(name):
    """(picture, derive(picture)) of a listed picture, made once and left unchanged."""
    if name not in _derived:
        pic = rc.picture(name)
        _derived[name] = (pic, rc.derive(pic))
    return _derived[name]


# ---------------------------------------------------------------------------------------------------------------- 1

def test_layouts_and_codes_match_the_header(tmp_path):
    text = open(HEADER).read()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vvc_mi355_rec.h"', "int main(void) {"]
    for cname, cls, size in MIRRORS:
        assert ctypes.sizeof(cls) == size
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{n} %zu\\n", offsetof({cname}, {n}));' for n, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for cname, cls, size in MIRRORS:
        assert int(got[cname]) == size
        for n, _ in cls._fields_:
            assert int(got[f"{cname}.{n}"]) == getattr(cls, n).offset, (cname, n)
    for size, what in ((32, "transform block"), (32, "transform unit"), (56, "coding unit"), (48, "picture's parameters")):
        assert re.search(r"%s; %d bytes, no implicit padding" % (what, size), text), what
    codes = _enum(text, "VVC355_REC_E_")
    assert len(codes) == len(CODES)
    for i, n in enumerate(CODES):
        assert codes["VVC355_REC_E_" + n] == getattr(abi, "REC_E_" + n) == -(i + 1), n
    assert _enum(text, "VVC355_REC_SLICE_") == dict(VVC355_REC_SLICE_DEP_QUANT=abi.REC_SLICE_DEP_QUANT, VVC355_REC_SLICE_LMCS=abi.REC_SLICE_LMCS)
    for name, sig in dict(rec_create=("p", ""), rec_destroy=("v", "p"), rec_begin_picture=("i", "pp"), rec_ctu=("i", "piipi"),
                          rec_end_picture=("i", "pp"), rec_fill_arena=("i", "pp"), rec_bind=("i", "pz")).items():
        assert abi.BATCH_SIGNATURES[name] == sig, name
    assert "one thread at a time" in text.lower() or "ONE thread at a time" in text
    # vvc_mi355.h and the context header are as they were: the recorder has its own header, which includes the first
    assert '#include "vvc_mi355.h"' in text and "vvc355_rec_" not in open(os.path.join(ROOT, "include", "vvc_mi355.h")).read()
    assert "vvc355_rec_" not in open(os.path.join(ROOT, "include", "vvc_mi355_ctx.h")).read()


# ---------------------------------------------------------------------------------------------------------------- 2, 3

def _check_equal(lib, pic, d):
    p = rk.pods(pic)
    for pack in (True, False):
        o = rk.record(lib, pic, pack, p=p)
        bad = rk.differences(lib, pic, d, o, pack)
        assert not bad, f"{pic.name}, packing {'on' if pack else 'off'}: {bad} differ from derive()"
        assert not o.cmds["pad_"].any(), "pad bytes of the commands"
        assert pcs.order_check(lib, o.ctus, pic.ncx, pic.ncy, o.order) == 0
        assert rc.order_defect(o.ctus, pic.ncx, pic.ncy, o.order) is None
        if pack and len(d.specs):
            assert (o.lv["flags"] & abi.LEVELS_INT32).sum() < len(o.lv), "no block of the picture is packed"
    return o


@pytest.mark.parametrize("name", rc.picture_names())
def test_listed_pictures_equal_derive(lib, name):
    pic, d = listed(name)
    _check_equal(lib, pic, d)


@pytest.mark.parametrize("k0", range(0, SWEEP, 8))
def test_sweep_pictures_equal_derive(lib, k0):
    for k in range(k0, k0 + 8):
        pic = rc.sweep_picture(k)
        _check_equal(lib, pic, rc.derive(pic))


def test_bind_turns_slots_into_addresses(lib):
    pic, _d = listed("T5")
    rec = lib.vvc355_rec_create()
    try:
        o = rk.record(lib, pic, True, rec=rec)
        is_res = o.cmds["kind"] == abi.RECON_RESID
        assert is_res.sum() > 10
        for base in (0x7F0000001000, 0x10000):               # again with another base: the slots are kept aside
            assert lib.vvc355_rec_bind(rec, base) == 0
            bound = rk._copy(o.res.cmds, o.res.n_cmds, rk.CMD)
            assert np.array_equal(bound["resid"][is_res], base + 4 * o.cmds["resid"][is_res]) and not bound["resid"][~is_res].any()
            rest = bound.copy()
            rest["resid"] = o.cmds["resid"]
            assert rest.tobytes() == o.cmds.tobytes()
    finally:
        lib.vvc355_rec_destroy(rec)


# ---------------------------------------------------------------------------------------------------------------- 4

@pytest.mark.parametrize("misread", rc.MISREADINGS)
def test_the_comparison_sees_every_misreading(lib, misread):
    assert rc.SENSITIVITY[misread]
    for name in rc.SENSITIVITY[misread]:
        pic, _d = listed(name)
        o = rk.record(lib, pic, True)
        assert rk.differences(lib, pic, rc.derive(pic, misread), o, True), f"{name}: the recorder equals derive() misread as {misread}"


# ---------------------------------------------------------------------------------------------------------------- 5

def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("cmds", "ctus", "order", "intra", "inter", "ts", "lv", "levels", "arena")) and \
        a.head == b.head


@pytest.mark.parametrize("name", ["T1", "T2", "T5", "T8"])
def test_ctus_in_any_order_give_the_same_result(lib, name):
    pic, _d = listed(name)
    p = rk.pods(pic)
    n = len(pic.ctus)
    raster = rk.record(lib, pic, True, p=p)
    for order in (np.arange(n)[::-1], np.random.default_rng(0x0DE2).permutation(n)):
        assert _same(raster, rk.record(lib, pic, True, order=order, p=p)), name


# ---------------------------------------------------------------------------------------------------------------- 6

def directed_picture(with_intra):
    """One CTU of 128: three inter units of 64x64, the one at (64, 0) with coded Cb and Cr, and a last unit at (64, 64) that is intra or inter."""
    pic = rc.draw("directed", 0xD1EC, bd=10, idc=1, ctb_log2=7, size=(128, 128), intra=0.0, slices=[(0, 1)], lmcs=True, inter_ctu=1.0)
    rng = np.random.default_rng(0xD1ED)
    sl = pic.slices[0]
    units = []
    for (x, y) in ((0, 0), (64, 0), (0, 64)):
        cu = rc._new_cu(x, y, 64, 64, 0)
        cu["qp"] = [30, 30, 30, 30]
        if (x, y) != (64, 0):
            cu["coded_flag"] = 0
        else:
            tu = dict(x0=x, y0=y, w=64, h=64, coded=[0, 1, 1], joint=0, tbs=[rc._tb(0, x, y, 64, 64, 0)])
            for c in (1, 2):
                lv, nzw, nzh = rc._levels(rng, pic, 32, 32, rc.tb_qp(pic, cu, tu, c, 0), sl[0], 0)
                tu["tbs"].append(rc._tb(c, x, y, 32, 32, 1, 0, lv, nzw, nzh))
            cu["tus"].append(tu)
        units.append(cu)
    units.append(rc._intra_cu(rng, pic, 64, 64, 64, 64, 0, sl) if with_intra else rc._inter_cu(rng, pic, 64, 64, 64, 64, sl))
    pic.ctus, pic._flat = [units], None
    return pic


def test_keep_is_decided_by_units_recorded_later(lib):
    late = 0
    for name in rc.picture_names():
        pic, _d = listed(name)
        late += rk.record(lib, pic, True).late_keep
    pic = directed_picture(True)
    o = _check_equal(lib, pic, rc.derive(pic))
    assert o.late_keep == 2 and o.stats == dict(keep=o.stats["keep"], batched_scaled=0, walk_scaled=2)
    chroma = o.inter[(o.inter["flags"] & 3) != 0]
    at_64 = chroma[(chroma["x0"] == 32) & (chroma["y0"] == 0)]
    assert len(at_64) == 2 and (at_64["flags"] & abi.INTER_TU_KEEP).all() and not (at_64["joint_mts"] & 15).any()
    resid = o.cmds[(o.cmds["kind"] == abi.RECON_RESID) & (o.cmds["x0"] == 64) & (o.cmds["y0"] == 0)]
    assert len(resid) == 2 and (resid["joint"] == 8).all()
    assert late + o.late_keep > 0
    # the same picture without the intra unit: the two blocks go to the batched pass, and the CTU has no commands
    pic = directed_picture(False)
    o = _check_equal(lib, pic, rc.derive(pic))
    chroma = o.inter[(o.inter["flags"] & 3) != 0]
    at_64 = chroma[(chroma["x0"] == 32) & (chroma["y0"] == 0)]
    assert len(at_64) == 2 and not (at_64["flags"] & abi.INTER_TU_KEEP).any() and ((at_64["joint_mts"] & 15) == 8).all()
    assert o.late_keep == 0 and o.stats["walk_scaled"] == 0 and o.stats["batched_scaled"] >= 2 and o.n_work == 0 and len(o.cmds) == 0


# ---------------------------------------------------------------------------------------------------------------- 7

def _refusal(lib, rec, pic, change, rs_list=None, n_cus=None):
    """Begin `pic`, apply `change` to a copy of its PODs, feed: the first code that is not 0."""
    p = rk.pods(pic)
    change(p)
    par = rk.params(pic)
    assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
    return rk.feed(lib, rec, pic, p, rs_list)


def test_refusals_leave_the_recorder_usable(lib):
    pic, d = listed("T5")
    fresh = rk.record(lib, pic, True)
    first, cus, tus, tbs, _lv = rc.shim_arrays(pic)
    coded = int(np.flatnonzero(tbs["has_coeffs"] != 0)[0])
    chroma = int(np.flatnonzero((tbs["has_coeffs"] != 0) & (tbs["c_idx"] > 0))[0])
    n = len(pic.ctus)

    def setf(arr, i, field, value):
        def change(p):
            getattr(p, arr)[field][i] = value
        return change

    cases = [
        (abi.REC_E_CTU_RANGE, lambda p: None, [n]),
        (abi.REC_E_CTU_RANGE, lambda p: None, [-1]),
        (abi.REC_E_CTU_TWICE, lambda p: None, [0, 1, 0]),
        (abi.REC_E_CU_RECT, setf("cus", 0, "x0", 64), None),                       # in the picture, outside CTU 0
        (abi.REC_E_CU_RECT, setf("cus", len(cus) - 1, "y0", pic.height), None),  # inside its CTU's square, outside the picture
        (abi.REC_E_SIDE, setf("cus", 0, "w", 24), None),
        (abi.REC_E_SIDE, setf("cus", 0, "w", 256), None),
        (abi.REC_E_SIDE, setf("tbs", coded, "w", 12), None),
        (abi.REC_E_SIDE, setf("tbs", coded, "h", 128), None),
        (abi.REC_E_TB_RECT, setf("tbs", coded, "x0", int(tbs["x0"][coded]) + 128), None),
        (abi.REC_E_TB_RECT, setf("tbs", coded, "max_x", 200), None),
        (abi.REC_E_C_IDX, setf("tbs", chroma, "c_idx", 3), None),
        (abi.REC_E_LEVELS, setf("tbs", coded, "levels", 0), None),
        (abi.REC_E_CIIP, setf("cus", 3, "ciip_flag", 1), None),
    ]
    rec = lib.vvc355_rec_create()
    try:
        res = abi.RecResult()
        assert lib.vvc355_rec_ctu(rec, 0, 0, None, 0) == abi.REC_E_STATE                        # no picture begun
        assert lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == abi.REC_E_STATE
        assert lib.vvc355_rec_bind(rec, 0) == abi.REC_E_STATE
        assert lib.vvc355_rec_begin_picture(rec, None) == abi.REC_E_ARGS and lib.vvc355_rec_begin_picture(None, None) == abi.REC_E_ARGS
        bad = rk.params(pic)
        bad.ctb_log2 = 8
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(bad)) == abi.REC_E_PARAMS
        for want, change, rs_list in cases:
            assert _refusal(lib, rec, pic, change, rs_list) == want, (want, rs_list)
            # the recorder is where begin_picture left it: the picture goes through the same object without another begin
            p = rk.pods(pic)
            assert rk.feed(lib, rec, pic, p) == 0
            assert lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
            assert _same(fresh, rk.snapshot(lib, rec, res)), want
            assert lib.vvc355_rec_ctu(rec, 0, 0, None, 0) == abi.REC_E_STATE                    # ended: a new picture has to begin
        # chroma blocks at 4:0:0
        mono, _dm = listed("T3")
        first_tb = int(np.flatnonzero(rc.shim_arrays(mono)[3]["has_coeffs"] != 0)[0])
        assert _refusal(lib, rec, mono, setf("tbs", first_tb, "c_idx", 1)) == abi.REC_E_C_IDX
        assert _same(rk.record(lib, mono, True), rk.record(lib, mono, True, rec=rec))
    finally:
        lib.vvc355_rec_destroy(rec)
    assert not rk.differences(lib, pic, d, fresh, True)


# ---------------------------------------------------------------------------------------------------------------- 8

# the runtimes linked in: the program then runs the same whatever else a machine loads into its processes
SAN_FLAGS = ["-std=c11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recorder_check")
    one = tmp / "one.c"
    one.write_text("int main(void) { return 0; }\n")
    flags = SAN_FLAGS
    if subprocess.run(["gcc", *flags, str(one), "-o", str(tmp / "one")], capture_output=True).returncode:
        flags = SAN_FLAGS[:-2]                                  # no static runtimes installed: the shared ones
        if subprocess.run(["gcc", *flags, str(one), "-o", str(tmp / "one")], capture_output=True).returncode:
            pytest.skip("gcc cannot build a one-line program with -fsanitize=address,undefined here")
    exe = tmp / "recorder_check"
    srcs = [os.path.join(ROOT, "tools", "recorder_check.c"), os.path.join(ROOT, "ffvvc_amd", "host", "recorder.c"),
            os.path.join(ROOT, "ffvvc_amd", "host", "levels_pack.c")]
    subprocess.check_call(["gcc", *flags, "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), *srcs, "-o", str(exe)])
    return exe, tmp


@pytest.mark.parametrize("name", ["T4", "T1", "T2"])          # dual tree; LMCS with tiles; 12 bit at range 18
def test_stand_alone_run_is_clean_under_the_sanitizers(lib, check_program, name):
    exe, tmp = check_program
    pic, d = listed(name)
    assert dict(T4=all(cu["tree_type"] for ctu in pic.ctus for cu in ctu), T1=pic.chroma_scale_flag and len(set(pic.col_bd[:-1].tolist())) > 1,
                T2=pic.bd == 12 and pic.rbits == 18)[name]
    path = tmp / f"{name}.dump"
    rk.dump(pic, path)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    want = "%016x" % rk.digest(rk.record(lib, pic, True))
    assert r.stdout.split() == [want, want], f"{name}: the stand-alone runs print {r.stdout.split()}, the library's run {want}"

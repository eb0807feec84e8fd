"""CPU: the ABI of vvc355_mvf_unit_pass — the layouts and codes as the header declares them, the frame validation (it precedes every HIP
call and therefore runs without a GPU, in a child process with a stream no runtime could use, so that a launch that should not have
happened cannot hide), the record predicate through vvc355_mvf_unit_check — and the expectations the GPU test compares with
(tests/mvf_unit_cases.py): the numpy restatement of the three storage rules against a scalar loop that follows vvc_mvs.c:282-491 line by
line with unbounded integers, values worked by hand, the digests of what the reference's own ff_vvc_store_sb_mvs / ff_vvc_store_gpm_mvf
wrote for the units of both sweeps (tests/golden/mvf_unit_ref.json), and the premises of the case lists, counted."""
import ctypes
import hashlib
import json
import subprocess
import sys

import numpy as np
import pytest

import mvf_unit_cases as mc
from conftest import ROOT
from ffvvc_amd import abi


@pytest.fixture(scope="module")
def lib():
    so = ctypes.CDLL(abi.LIB_PATH)
    so.vvc355_mvf_unit_check.restype = ctypes.c_int
    so.vvc355_mvf_unit_check.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return so


def test_layouts_match_the_header():
    assert ctypes.sizeof(abi.MvfUnit) == 64 and ctypes.sizeof(abi.MvfUnitFrame) == 64
    offs = {n: getattr(abi.MvfUnit, n).offset for n, _ in abi.MvfUnit._fields_}
    assert offs == dict(x0=0, y0=2, w=4, h=5, kind=6, aux=7, link=8, pf=12, ref_idx=13, pad_=15, body=16)
    assert {n: mc.UNIT_DT.fields[n][1] for n in mc.UNIT_DT.names} == offs
    offs = {n: getattr(abi.MvfUnitFrame, n).offset for n, _ in abi.MvfUnitFrame._fields_}
    assert offs == dict(units=0, ctu_first=8, mvf=16, affine_cus=24, n_units=32, n_affine_cus=36, mvf_pitch=40, width=44, height=48,
                        ctb_width=52, ctb_height=56, ctb_log2=60, prof_disabled=61, pad_=62)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    assert "} vvc355_mvf_unit;" in text and "} vvc355_mvf_unit_frame;" in text and "the record is 64 bytes (16-byte aligned in the array), the frame 64" in text
    assert "enum { VVC355_MVF_PLAIN = 0, VVC355_MVF_AFFINE = 1, VVC355_MVF_GPM = 2 };" in text and "#define VVC355_MVF_LINK_NONE 0xFFFFFFFFu" in text
    assert (abi.MVF_PLAIN, abi.MVF_AFFINE, abi.MVF_GPM, abi.MVF_LINK_NONE) == (0, 1, 2, 0xFFFFFFFF)
    assert abi.BATCH_SIGNATURES["mvf_unit_pass"] == ("i", "ppp") and abi.BATCH_SIGNATURES["mvf_unit_check"] == ("i", "ppi")
    # the fields of vvc355_affine_cu the pass writes
    assert abi.AffineCu.prof_flags.offset == 10 and abi.AffineCu.diff_mv.offset == 16 and ctypes.sizeof(abi.AffineCu) == 144


E_CODES = ("FRAME", "SIZE", "COUNT", "CTB", "GRID", "PITCH", "RECORDS", "AFFINE")
R_CODES = ("SIDE", "PLACE", "CTU", "PAD", "KIND", "AFF_SHAPE", "AFF_MODEL", "AFF_PRED", "AFF_LINK", "GPM_SHAPE", "GPM_RATIO", "GPM_PART", "GPM_PRED")


def test_codes_are_distinct_and_the_headers():
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    e = [getattr(abi, "MVF_UNIT_E_" + n) for n in E_CODES]
    assert all(c < 0 for c in e) and len(set(e)) == len(e)
    for n, c in zip(E_CODES, e):
        assert f"VVC355_MVF_UNIT_E_{n} = {c}" in text, n
    r = [getattr(abi, "MVF_UNIT_R_" + n) for n in R_CODES]
    assert all(c > 0 for c in r) and len(set(r)) == len(r)
    for n, c in zip(R_CODES, r):
        assert f"VVC355_MVF_UNIT_R_{n} = {c}" in text, n


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_mvf_unit_pass.restype = ctypes.c_int
lib.vvc355_mvf_unit_pass.argtypes = [ctypes.c_void_p] * 3
STREAM = 0xdead0001          # no runtime could use it: a launch would fault or fail loudly

def frame(**kw):
    f = abi.MvfUnitFrame()
    f.units, f.ctu_first, f.mvf, f.affine_cus, f.n_units, f.n_affine_cus = 0x1000, 0x2000, 0x3000, 0x4000, 10, 3
    f.width, f.height, f.ctb_log2, f.ctb_width, f.ctb_height, f.mvf_pitch = 328, 200, 6, 6, 4, 82
    for k, v in kw.items():
        setattr(f, k, v)
    return f

def run(f):
    return lib.vvc355_mvf_unit_pass(STREAM, 0xf000, ctypes.addressof(f))

assert lib.vvc355_mvf_unit_pass(STREAM, 0xf000, None) == abi.MVF_UNIT_E_FRAME, "no host frame"
assert lib.vvc355_mvf_unit_pass(STREAM, None, ctypes.addressof(frame())) == abi.MVF_UNIT_E_FRAME, "no device frame"
for kw in (dict(width=0), dict(width=-8), dict(height=0), dict(width=330), dict(height=202), dict(width=32768)):
    assert run(frame(**kw)) == abi.MVF_UNIT_E_SIZE, kw
for kw in (dict(n_units=-1), dict(n_affine_cus=-1)):
    assert run(frame(**kw)) == abi.MVF_UNIT_E_COUNT, kw
for v in (4, 8, 0):
    assert run(frame(ctb_log2=v)) == abi.MVF_UNIT_E_CTB, v
for kw in (dict(ctb_width=5), dict(ctb_width=7), dict(ctb_height=3), dict(ctb_height=5), dict(ctb_log2=7), dict(ctb_log2=5)):
    assert run(frame(**kw)) == abi.MVF_UNIT_E_GRID, kw
for v in (81, 0, -82):
    assert run(frame(mvf_pitch=v)) == abi.MVF_UNIT_E_PITCH, v
for kw in (dict(units=0), dict(ctu_first=0), dict(mvf=0), dict(units=0x1008), dict(ctu_first=0x2002), dict(mvf=0x3004)):
    assert run(frame(**kw)) == abi.MVF_UNIT_E_RECORDS, kw
for kw in (dict(affine_cus=0), dict(affine_cus=0x4002)):
    assert run(frame(**kw)) == abi.MVF_UNIT_E_AFFINE, kw
# the order: of two faults the one checked first is reported
assert run(frame(width=0, n_units=-1)) == abi.MVF_UNIT_E_SIZE and run(frame(n_units=-1, ctb_log2=9)) == abi.MVF_UNIT_E_COUNT
assert run(frame(ctb_log2=9, ctb_width=0)) == abi.MVF_UNIT_E_CTB and run(frame(ctb_width=0, mvf_pitch=0)) == abi.MVF_UNIT_E_GRID
assert run(frame(mvf_pitch=0, units=0)) == abi.MVF_UNIT_E_PITCH and run(frame(units=0, affine_cus=0)) == abi.MVF_UNIT_E_RECORDS
# nothing to do is not a fault, and launches nothing: no records (their arrays may then be missing), no affine records to link
assert run(frame(n_units=0, units=0, ctu_first=0, mvf=0)) == 0
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    assert b"validated" in r.stdout


# ------------------------------------------------------------------------------------------------------------------ the record check

G = mc.Geo(200, 136, 6)              # 4 x 3 CTUs of 64, partial right (8 wide) and bottom (8 high)


def _frame(g, n_cus=4):
    return mc.unit_frame(g, 0, 0, 0, 0, g.tw, 0, n_cus)


def _check(lib, g, rec, rs, n_cus=4):
    f = _frame(g, n_cus)
    a = np.array(rec, mc.UNIT_DT).reshape(1)
    got = lib.vvc355_mvf_unit_check(a.ctypes.data, ctypes.addressof(f), rs)
    assert got == mc.rule(g, a[0], rs, n_cus), "the numpy side's predicate disagrees with the library's"
    return got


def _m(pf):
    return mc.mvfield(pred_flag=pf)


def _with(rec, **kw):
    r = rec.copy()
    for k, v in kw.items():
        r[k] = v
    return r


def test_malformed_records_name_their_rule(lib):
    cp = np.arange(12).reshape(2, 3, 2)
    P, A, M = mc.plain(64, 64, 16, 8, _m(1)), mc.affine(64, 64, 16, 8, 1, 3, cp, link=1), mc.gpm(64, 64, 16, 8, 5, _m(1), _m(2))
    rs = 5                            # CTU (1, 1)
    for good in (P, A, M):
        assert _check(lib, G, good, rs) == 0
    R = {n: getattr(abi, "MVF_UNIT_R_" + n) for n in R_CODES}
    for rec in (P, A, M):
        for kw in (dict(w=0), dict(h=0), dict(w=6), dict(h=10), dict(w=132), dict(h=136), dict(w=255)):
            assert _check(lib, G, _with(rec, **kw), rs) == R["SIDE"], kw
        for kw in (dict(x0=-4), dict(y0=-64), dict(x0=66), dict(y0=65), dict(x0=192), dict(y0=132), dict(x0=200), dict(y0=136)):
            assert _check(lib, G, _with(rec, **kw), 0 if kw.get("x0", 0) < 0 or kw.get("y0", 0) < 0 else rs) == R["PLACE"], kw
        for kw in (dict(x0=120), dict(y0=124), dict(x0=48), dict(y0=56), dict(x0=128), dict(y0=0)):
            assert _check(lib, G, _with(rec, **kw), rs) == R["CTU"], kw
        assert _check(lib, G, rec, rs + 1) == R["CTU"] and _check(lib, G, rec, 0) == R["CTU"]            # filed under the wrong CTU
        assert _check(lib, G, _with(rec, pad_=1), rs) == R["PAD"] and _check(lib, G, _with(rec, pad_=128), rs) == R["PAD"]
        assert _check(lib, G, _with(rec, kind=3), rs) == R["KIND"] and _check(lib, G, _with(rec, kind=255), rs) == R["KIND"]
    for kw in (dict(w=4), dict(h=4), dict(w=12), dict(h=24), dict(w=48, x0=64)):
        assert _check(lib, G, _with(A, **kw), rs) == R["AFF_SHAPE"], kw
    for v in (0, 3, 255):
        assert _check(lib, G, _with(A, aux=v), rs) == R["AFF_MODEL"], v
    for v in (0, 0x7C):
        assert _check(lib, G, _with(A, pf=v), rs) == R["AFF_PRED"], v
    for v in (4, 5, 0xFFFFFFFE):
        assert _check(lib, G, _with(A, link=v), rs) == R["AFF_LINK"], v
    assert _check(lib, G, _with(A, link=0), rs, n_cus=0) == R["AFF_LINK"] and _check(lib, G, _with(A, link=mc.NONE), rs, n_cus=0) == 0
    assert _check(lib, G, _with(A, link=3), rs) == 0
    for kw in (dict(w=4), dict(h=4)):
        assert _check(lib, G, _with(M, **kw), rs) == R["GPM_SHAPE"], kw
    g128 = mc.Geo(256, 128, 7)
    assert _check(lib, g128, mc.gpm(0, 0, 128, 64, 5, _m(1), _m(2)), 0) == R["GPM_SHAPE"] and _check(lib, g128, mc.gpm(0, 0, 64, 128, 5, _m(1), _m(2)), 0) == R["GPM_SHAPE"]
    assert _check(lib, G, mc.gpm(64, 64, 64, 8, 5, _m(1), _m(2)), rs) == R["GPM_RATIO"] and _check(lib, G, mc.gpm(64, 64, 8, 64, 5, _m(1), _m(2)), rs) == R["GPM_RATIO"]
    assert _check(lib, G, mc.gpm(64, 64, 32, 8, 5, _m(1), _m(2)), rs) == 0 and _check(lib, G, mc.gpm(64, 64, 12, 8, 5, _m(1), _m(2)), rs) == 0
    for v in (64, 255):
        assert _check(lib, G, _with(M, aux=v), rs) == R["GPM_PART"], v
    for a, b in ((0, 1), (3, 1), (1, 0), (2, 3), (4, 2)):
        assert _check(lib, G, mc.gpm(64, 64, 16, 8, 5, _m(a), _m(b)), rs) == R["GPM_PRED"], (a, b)
    # fields another kind owns are not looked at
    assert _check(lib, G, _with(P, aux=99, link=77, pf=0), rs) == 0 and _check(lib, G, _with(M, link=77, pf=0), rs) == 0
    # no record, no frame, a CTU outside the grid
    f = _frame(G)
    one = np.array(P, mc.UNIT_DT).reshape(1)
    assert lib.vvc355_mvf_unit_check(None, ctypes.addressof(f), 0) == -1 and lib.vvc355_mvf_unit_check(one.ctypes.data, None, 0) == -1
    assert lib.vvc355_mvf_unit_check(one.ctypes.data, ctypes.addressof(f), 12) == -1 and lib.vvc355_mvf_unit_check(one.ctypes.data, ctypes.addressof(f), -1) == -1


def test_legal_records_at_the_pictures_right_and_bottom_edge(lib):
    cp = np.zeros((2, 3, 2), int)
    for rec, rs in ((mc.plain(192, 0, 8, 64, _m(1)), 3), (mc.plain(196, 132, 4, 4, _m(0)), 11), (mc.plain(0, 128, 64, 8, _m(3)), 8),
                    (mc.affine(192, 64, 8, 64, 2, 1, cp), 7), (mc.affine(128, 128, 64, 8, 1, 2, cp), 10), (mc.affine(192, 128, 8, 8, 1, 3, cp, link=0), 11),
                    (mc.gpm(192, 32, 8, 32, 63, _m(2), _m(2)), 3), (mc.gpm(64, 128, 32, 8, 0, _m(1), _m(1)), 9), (mc.gpm(192, 128, 8, 8, 17, _m(2), _m(1)), 11)):
        assert _check(lib, G, rec, rs) == 0, rec
        x0, y0, w, h = (int(rec[k]) for k in ("x0", "y0", "w", "h"))
        assert x0 + w == G.width or y0 + h == G.height
        if x0 + w == G.width:
            assert _check(lib, G, _with(rec, x0=x0 + 4), rs) == abi.MVF_UNIT_R_PLACE
        if y0 + h == G.height:
            assert _check(lib, G, _with(rec, y0=y0 + 4), rs) == abi.MVF_UNIT_R_PLACE


# --------------------------------------------------------------------------------------------------------- the expectations

def test_values_worked_by_hand():
    # 4 parameters, 16x8, list 0: cp0 = (100, -50), cp1 = (116, -42): d_hor_x = 16 * 8 = 128, d_ver_x = 8 * 8 = 64, d_hor_y = -64, d_ver_y = 128,
    # scale = (12800, -6400).  Sub-block (sbx, sby) at (2 + 4 sbx, 2 + 4 sby): x = 12800 + 128 xp - 64 yp, y = -6400 + 64 xp + 128 yp:
    #   (0, 0): (12928, -6016) -> (101, -47)     (3, 0): (14464, -5248) -> (113, -41)     (0, 1): (12672, -5504) -> (99, -43)     (3, 1): (14208, -4736) -> (111, -37)
    # diff_mv: 4 d = (512, 256 | -256, 512), offsets 6 * (128 - 64) = 384 and 6 * (64 + 128) = 1152: x = 0, y = 0 -> (-384, -1152) -> (-1.5, -4.5)
    # -> (-1, -4); x = 3, y = 3 -> (384, 1152) -> (1.5, 4.5) -> (1, 4): halves round towards zero on both sides, (v + 128) >> 8 would give (-1, -4) and (2, 5)
    cp = [[(100, -50), (116, -42), (7, 7)], [(0, 0)] * 3]
    e, flags, dmv, facts = mc.affine_unit(mc.affine(0, 0, 16, 8, 1, 1, cp, ref_idx=(2, -1), hpel=1))
    assert e["mv"][:, :, 0].tolist() == [[[101, -47], [105, -45], [109, -43], [113, -41]], [[99, -43], [103, -41], [107, -39], [111, -37]]]
    assert not e["mv"][:, :, 1].any() and set(e["pred_flag"].ravel()) == {1} and set(e["hpel_if_idx"].ravel()) == {1} and e["ref_idx"][1, 2].tolist() == [2, -1]
    assert flags == 1 and not facts[0]["fallback"] and not dmv[1].any()
    assert (dmv[0, 0, 0], dmv[0, 1, 0], dmv[0, 0, 15], dmv[0, 1, 15]) == (-1, -4, 1, 4)
    assert dmv[0, 0].tolist() == [-1, 0, 2, 4, -2, 0, 1, 3, -3, -1, 0, 2, -4, -2, 0, 1]
    # 6 parameters, 8x16, list 1, bi-predicted with list 0 at rest: cp = (0, 0), (640, 0), (0, -40): d_hor_x = 640 * 16 = 10240, d_ver_x = 0,
    # d_hor_y = 0, d_ver_y = -40 * 8 = -320.  a = 4 * 12288 = 49152, b = 0, c = 4 * 1728 = 6912, d = 0: (49152 >> 11) + 9 = 33, (6912 >> 11) + 9 = 12,
    # 396 > 225: fallback, every sub-block at (4, 8): (40960, -2560) -> (320, -20); no PROF.  List 0: equal control points, no fallback, no PROF.
    cp = [[(-9, 9)] * 3, [(0, 0), (640, 0), (0, -40)]]
    e, flags, dmv, facts = mc.affine_unit(mc.affine(0, 0, 8, 16, 2, 3, cp, bcw=2))
    assert facts[1]["fallback"] and not facts[0]["fallback"] and flags == 0 and not dmv.any()
    assert np.all(e["mv"][:, :, 1] == (320, -20)) and np.all(e["mv"][:, :, 0] == (-9, 9)) and set(e["bcw_idx"].ravel()) == {2} and e.shape == (4, 2)
    # GPM 8x8, partition 10: angle 4, distance 0, disLut[4] = 4, disLut[12] = -4, no flip; angle % 16 = 4 and h >= w: shift_hor = 0; offsets (-4, -4)
    # motion_idx = (2 (x - 4) + 5) * 4 - (2 (y - 4) + 5) * 4 = 8 (x - y): 0 on the diagonal (s_type 2), -32 at (0, 4) (s_type 1), 32 at (4, 0) (0)
    s_type, is_flip, shift_hor = mc.gpm_types(8, 8, 10)
    assert s_type.tolist() == [[2, 0], [1, 2]] and (is_flip, shift_hor) == (0, 0)
    m0 = mc.mvfield(mv=((5, 6), (0, 0)), ref_idx=(1, -1), pred_flag=1, hpel=1, pad=(9, 9))
    m1 = mc.mvfield(mv=((0, 0), (-7, 8)), ref_idx=(-1, 2), pred_flag=2)
    e, _ = mc.gpm_unit(mc.gpm(0, 0, 8, 8, 10, m0, m1))
    assert e[0, 1] == m0 and e[1, 0] == m1
    both = mc.mvfield(mv=((5, 6), (-7, 8)), ref_idx=(1, 2), pred_flag=3, hpel=1, pad=(9, 9))
    assert e[0, 0] == both and e[1, 1] == both
    e, _ = mc.gpm_unit(mc.gpm(0, 0, 8, 8, 10, m0, mc.mvfield(mv=((1, 2), (0, 0)), ref_idx=(0, -1), pred_flag=1)))          # the same list: gpm_mv[1] on the diagonal
    assert e[0, 0]["mv"][0].tolist() == [1, 2] and e[0, 0]["pred_flag"] == 1 and e[0, 1] == m0


def _all_affine():
    for shape in mc.AFFINE_SHAPES:
        for (g, units, first) in mc.affine_pictures(shape):
            for r in units:
                yield r


def test_numpy_restatement_equals_the_scalar_loop():
    """Every unit of the affine sweep up to 32x32, a sample of the larger ones, every GPM shape with every partition: all entries, flags and
    offsets.  The scalar loop computes with unbounded integers and records the widest value an int of the reference would have held."""
    widest = mc.Widest()
    n = 0
    for k, r in enumerate(_all_affine()):
        if int(r["w"]) * int(r["h"]) > 1024 and k % 5:
            continue
        for prof_disabled in (0, 1):
            e, flags, dmv, _ = mc.affine_unit(r, prof_disabled)
            out, sflags, sdiff = mc.scalar_unit(r, prof_disabled, widest)
            assert len(out) == e.size and all(out[(4 * x, 4 * y)] == e[y, x] for y in range(e.shape[0]) for x in range(e.shape[1])), r
            assert flags == sflags[0] | sflags[1] << 1 and np.array_equal(dmv, sdiff), r
        n += 1
    assert n > 400
    for shape in mc.GPM_SHAPES:
        for (g, units, first) in mc.gpm_pictures(shape):
            for r in units[::3]:
                e, _ = mc.gpm_unit(r)
                out, _, _ = mc.scalar_unit(r, 0, widest)
                assert len(out) == e.size and all(out[(4 * x, 4 * y)] == e[y, x] for y in range(e.shape[0]) for x in range(e.shape[1])), r
    # the domain: the reference is not built with -fwrapv; nothing it computes on these cases leaves an int
    assert 1 << 24 < widest.v < 1 << 31, widest.v


def test_numpy_restatement_reproduces_the_references_digests():
    """tests/golden/mvf_unit_ref.json (tests/golden/mvf_unit_ref.md says how it was made): per shape the units of the affine sweep (PROF allowed, then switched off) and of the GPM sweep, through
    the reference's own functions; the numpy side hashes to the same digests, and the generator still draws the same inputs."""
    golden = json.load(open(f"{ROOT}/tests/golden/mvf_unit_ref.json"))
    groups = mc.ref_groups()
    assert set(golden) == set(groups) and len(groups) == 25 + 14
    for name, cases in groups.items():
        assert golden[name]["cases"] == len(cases), name
        assert hashlib.sha256(mc.ref_inputs(cases)).hexdigest() == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
        assert hashlib.sha256(mc.ref_outputs(cases)).hexdigest() == golden[name]["outputs"], f"{name}: the numpy side differs from what the reference wrote"
    assert sum(g["cases"] for g in golden.values()) == 2 * sum(len(mc.affine_params(*s)) for s in mc.AFFINE_SHAPES) + 14 * 256


def test_the_whole_affine_sweep_stays_inside_int():
    """All units (the scalar loop above samples the large ones): the numpy side computes in int64; its widest sums bound the reference's."""
    for r in _all_affine():
        cp = mc.unit_cp(r)
        assert cp.min() >= mc.MV_MIN and cp.max() <= mc.MV_MAX
        _, _, _, facts = mc.affine_unit(r)
        for f in facts.values():
            assert max(int(np.abs(f["pre"][0]).max()), int(np.abs(f["pre"][1]).max())) + 64 < 1 << 31


def test_premises_of_the_affine_case_list():
    seen = set()
    lo = hi = dlo = dhi = neg_half = 0
    for r in _all_affine():
        model, pred = int(r["aux"]), int(r["pf"]) & 3
        _, flags, dmv, facts = mc.affine_unit(r)
        _, flags_off, dmv_off, _ = mc.affine_unit(r, 1)
        assert flags_off == 0 and not dmv_off.any()
        fb = [f["fallback"] for f in facts.values()]
        seen.add(("fallback", pred == 3, any(fb)))
        seen.add(("no fallback", pred == 3, not all(fb)))
        if pred == 3 and fb[0] != fb[1]:
            seen.add("lists decide differently")
        for l, f in facts.items():
            cp = mc.unit_cp(r)[l].tolist()
            equal = cp[0] == cp[1] and (model == 1 or cp[0] == cp[2])
            if equal and not f["fallback"]:
                assert not f["flag"]
                seen.add(("PROF off: equal control points", model))
            if model == 2 and cp[0] == cp[1] and cp[0] != cp[2] and not f["fallback"]:
                assert f["flag"]
                seen.add("6 parameters: only the first two equal keeps PROF")
            if f["fallback"] and not equal:
                assert not f["flag"]
                seen.add("PROF off: fallback")
            if f["flag"]:
                seen.add("PROF on")
                dlo += int(np.count_nonzero(f["raw_d"] < -31))
                dhi += int(np.count_nonzero(f["raw_d"] > 31))
                seen.add("PROF off: prof_disabled")              # (flags_off above: this unit's flag is 0 with the switch)
            lo += int(np.count_nonzero(f["raw"] < mc.MV_MIN))
            hi += int(np.count_nonzero(f["raw"] > mc.MV_MAX))
            for v in f["pre"]:
                neg_half += int(np.count_nonzero((v < 0) & ((v + 64) % 128 == 0)))          # (v + 64) >> 7 would round these the other way
    want = {(k, bi, True) for k in ("fallback", "no fallback") for bi in (False, True)} | {
        "lists decide differently", ("PROF off: equal control points", 1), ("PROF off: equal control points", 2),
        "6 parameters: only the first two equal keeps PROF", "PROF off: fallback", "PROF off: prof_disabled", "PROF on"}
    assert want <= seen, want - seen
    assert lo > 0 and hi > 0, "both bounds of the 18-bit clip"
    assert dlo > 0 and dhi > 0, "both bounds of the +-31 clip"
    assert neg_half > 0, "negative values that round differently from a plain shift"


def test_premises_of_the_gpm_case_list():
    types, flips, shifts, combos = set(), set(), set(), set()
    n = 0
    for shape in mc.GPM_SHAPES:
        for (g, units, first) in mc.gpm_pictures(shape):
            n += len(units)
            for r in units:
                s_type, is_flip, shift_hor = mc.gpm_types(int(r["w"]), int(r["h"]), int(r["aux"]))
                m0, m1 = r["body"].view(mc.MVF_DT)
                flips.add(is_flip)
                shifts.add(shift_hor)
                types |= set(s_type.ravel().tolist())
                if 2 in s_type:
                    combos.add("BI" if int(m0["pred_flag"]) != int(m1["pred_flag"]) else "same list")
                assert m0["pad_"].all() and m1["pad_"].all()                  # pad bytes that a verbatim copy must carry
    assert n == 14 * 64 * 4 and types == {0, 1, 2} and flips == {0, 1} and shifts == {0, 1} and combos == {"BI", "same list"}


def test_premises_of_the_pictures():
    for ctb_log2 in (5, 6, 7):
        g, units, first = mc.plain_picture(ctb_log2)
        assert (g.width, g.height) == (136, 72) and g.width % (1 << ctb_log2) and g.height % (1 << ctb_log2)
        sizes = set(zip(units["w"].tolist(), units["h"].tolist()))
        assert {(4, 4), (4, 8), (8, 4)} <= sizes and (min(1 << ctb_log2, 128), min(1 << ctb_log2, 72)) in sizes
        assert mc.placed(g, units, first, 0).all()
        cover = np.zeros((g.th, g.tw), int)
        for r in units:
            cover[r["y0"] // 4:(r["y0"] + int(r["h"])) // 4, r["x0"] // 4:(r["x0"] + int(r["w"])) // 4] += 1
        assert np.all(cover == 1)                                             # the units tile the picture: the edges that are no multiple of the CTU too
    g, units, first = mc.plain_picture(7, 136, 136)
    assert (128, 128) in set(zip(units["w"].tolist(), units["h"].tolist()))
    for shape in mc.AFFINE_SHAPES:
        pics = mc.affine_pictures(shape)
        assert sum(len(u) for _, u, _ in pics) == len(mc.affine_params(*shape)) >= 24
        assert all(mc.placed(g, u, f, len(u)).all() for g, u, f in pics)
    for shape in mc.GPM_SHAPES:
        assert all(mc.placed(g, u, f, 0).all() for g, u, f in mc.gpm_pictures(shape))


def test_expansion_is_the_table(orc):
    """The vvc355_mv_rec list of a mixed picture, painted by the table setters' definition, is the numpy table; without merging it holds one
    record per 4x4 block of every AFFINE and GPM unit."""
    import bs_cases
    t = bs_cases.BsTables(np.random.default_rng(mc.SEED + 3), 200, 136, ctb_log2=6)
    g, units, first, n_aff = mc.mixed_picture([c[:4] for c in t.cu_recs])
    kinds = units["kind"].tolist()
    assert min(kinds.count(k) for k in (mc.PLAIN, mc.AFFINE, mc.GPM)) >= 5 and mc.placed(g, units, first, n_aff).all()
    want = np.zeros((g.th, g.tw), mc.MVF_DT)
    mc.expect_table(g, units, first, want, n_aff)
    for merge in (True, False):
        recs, rfirst = mc.expand(g, units, first, n_aff, merge)
        got = np.zeros((g.th, g.tw), mc.MVF_DT)
        for r in recs:
            got[r["y0"] // 4:(r["y0"] + int(r["h"])) // 4, r["x0"] // 4:(r["x0"] + int(r["w"])) // 4] = np.frombuffer(r["mvf"].tobytes(), mc.MVF_DT)[0]
        assert np.array_equal(got, want) and rfirst[-1] == len(recs)
    sub = units[units["kind"] != mc.PLAIN]
    assert len(recs) == int(np.count_nonzero(units["kind"] == mc.PLAIN)) + int(np.sum(sub["w"].astype(int) * sub["h"].astype(int))) // 16
    assert np.any(want["pred_flag"] == 0) and np.all(want["pred_flag"] <= 3)

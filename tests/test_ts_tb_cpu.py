"""CPU: the ABI of vvc355_ts_tb_pass — record and frame layouts as the header declares them, the frame validation, which precedes every HIP
call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot hide), and the case
module's own premises: the saturating BDPCM levels tell the reference's clipped running sum from a plain prefix sum, in both directions
and at both ends of the range, by the oracle alone."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import ts_tb_cases as ts
from conftest import ROOT
from ffvvc_amd import abi


def test_record_and_frame_layouts_match_the_header():
    assert ctypes.sizeof(abi.TsTu) == 16
    offs = {n: getattr(abi.TsTu, n).offset for n, _ in abi.TsTu._fields_}
    assert offs == dict(coeff_off=0, x0=4, y0=6, log2_w=8, log2_h=9, nzw=10, nzh=11, qp=12, pad_=13, flags=14, joint=15)
    # what means the same sits where vvc355_inter_tu has it
    for mine, theirs in (("coeff_off", "coeff_off"), ("x0", "x0"), ("y0", "y0"), ("log2_w", "log2_w"), ("log2_h", "log2_h"), ("nzw", "nzw"),
                         ("nzh", "nzh"), ("qp", "qp"), ("flags", "flags"), ("joint", "joint_mts")):
        assert getattr(abi.TsTu, mine).offset == getattr(abi.InterTu, theirs).offset
    assert (abi.TS_TU_KEEP, abi.TS_TU_UNIT_DX, abi.TS_TU_UNIT_DY) == (abi.INTER_TU_KEEP, abi.INTER_TU_UNIT_DX, abi.INTER_TU_UNIT_DY)
    assert (abi.TS_TU_BDPCM, abi.TS_TU_VERTICAL) == (4, 64)
    assert ctypes.sizeof(abi.TsTbFrame) == 136
    offs = {n: getattr(abi.TsTbFrame, n).offset for n, _ in abi.TsTbFrame._fields_}
    assert offs == dict(tus=0, coeffs=8, lv=16, levels=24, plane=32, scale_table=56, stride=64, width=76, height=80, n_tus=84, hs=88, vs=89,
                        size_y=90, range=91, bd=92, pad_=93, class_first=96)
    assert abi.BATCH_SIGNATURES["ts_tb_pass"] == ("i", "pppi")
    # the header's own words: field order of both structs, the flag bits and the number of classes
    hdr = open(f"{ROOT}/include/vvc_mi355.h").read()
    for name, cls in (("vvc355_ts_tu", abi.TsTu), ("vvc355_ts_tb_frame", abi.TsTbFrame)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [n for n, _ in cls._fields_], name
    enums = dict(re.findall(r"(VVC355_TS_T[UB]_\w+) = (-?\d+)", hdr))
    assert {k: int(v) for k, v in enums.items()} == dict(
        VVC355_TS_TU_BDPCM=abi.TS_TU_BDPCM, VVC355_TS_TU_KEEP=abi.TS_TU_KEEP, VVC355_TS_TU_UNIT_DX=abi.TS_TU_UNIT_DX,
        VVC355_TS_TU_UNIT_DY=abi.TS_TU_UNIT_DY, VVC355_TS_TU_VERTICAL=abi.TS_TU_VERTICAL, VVC355_TS_TB_CLASSES=abi.TS_TB_CLASSES,
        VVC355_TS_TB_E_CLASS=abi.TS_TB_E_CLASS, VVC355_TS_TB_E_BD=abi.TS_TB_E_BD, VVC355_TS_TB_E_RANGE=abi.TS_TB_E_RANGE,
        VVC355_TS_TB_E_LEVELS=abi.TS_TB_E_LEVELS, VVC355_TS_TB_E_SIZE_Y=abi.TS_TB_E_SIZE_Y, VVC355_TS_TB_E_SHIFT=abi.TS_TB_E_SHIFT,
        VVC355_TS_TB_E_CHANNELS=abi.TS_TB_E_CHANNELS, VVC355_TS_TB_E_ORDER=abi.TS_TB_E_ORDER)


def test_error_codes_are_distinct_and_negative():
    codes = [abi.TS_TB_E_CLASS, abi.TS_TB_E_BD, abi.TS_TB_E_RANGE, abi.TS_TB_E_LEVELS, abi.TS_TB_E_SIZE_Y, abi.TS_TB_E_SHIFT,
             abi.TS_TB_E_CHANNELS, abi.TS_TB_E_ORDER]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_ts_tb_pass.restype = ctypes.c_int
lib.vvc355_ts_tb_pass.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]
NC = abi.TS_TB_CLASSES

def frame(n=2 * NC, cf=None, bd=10, rng=15, lv=0, levels=0, table=0, size_y=64, hs=1, vs=1):
    f = abi.TsTbFrame()
    f.tus, f.coeffs, f.lv, f.levels, f.n_tus, f.scale_table = 0x1000, 0x2000, lv, levels, n, table
    for c in range(3):
        f.plane[c], f.stride[c] = 0x10000 * (c + 1), 512
    f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = 256, 128, hs, vs, size_y, rng, bd
    if cf is None:
        cf = [list(range(NC + 1)), list(range(NC, 2 * NC + 1))]     # one record per class: 0..4 | 4..8
    for ch in range(2):
        for k in range(NC + 1):
            f.class_first[ch][k] = cf[ch][k]
    return f

def run(f, channels=3):
    return lib.vvc355_ts_tb_pass(None, 0x3000, ctypes.addressof(f), channels)

def classes(edit):
    b = [list(range(NC + 1)), list(range(NC, 2 * NC + 1))]
    edit(b)
    return b

def swap(b): b[0][2], b[0][3] = b[0][3], b[0][2]
def gap(b): b[1][0] += 1
def short(b): b[1][NC] -= 1
def first(b): b[0][0] = 1
def chroma_down(b): b[1][2] = b[1][1] - 1

assert run(frame(cf=classes(swap))) == abi.TS_TB_E_CLASS, "luma classes not monotonic"
assert run(frame(cf=classes(chroma_down))) == abi.TS_TB_E_CLASS, "chroma classes not monotonic"
assert run(frame(cf=classes(gap))) == abi.TS_TB_E_CLASS, "chroma does not start where luma ends"
assert run(frame(cf=classes(short))) == abi.TS_TB_E_CLASS, "last class does not end at n_tus"
assert run(frame(cf=classes(first))) == abi.TS_TB_E_CLASS, "first class does not start at 0"
assert run(frame(n=-1, cf=[[0] * (NC + 1), [0] * NC + [-1]])) == abi.TS_TB_E_CLASS
assert lib.vvc355_ts_tb_pass(None, 0x3000, None, 3) == abi.TS_TB_E_CLASS, "no host frame"
assert run(frame(bd=9)) == abi.TS_TB_E_BD
assert run(frame(bd=16)) == abi.TS_TB_E_BD
assert run(frame(rng=14)) == abi.TS_TB_E_RANGE
assert run(frame(rng=21)) == abi.TS_TB_E_RANGE
assert run(frame(lv=0x4000)) == abi.TS_TB_E_LEVELS, "lv without levels"
assert run(frame(levels=0x4000)) == abi.TS_TB_E_LEVELS, "levels without lv"
assert run(frame(table=0x5000, size_y=128), 2) == abi.TS_TB_E_SIZE_Y
assert run(frame(table=0x5000, size_y=16), 1) == abi.TS_TB_E_SIZE_Y
assert run(frame(hs=2)) == abi.TS_TB_E_SHIFT
assert run(frame(vs=2)) == abi.TS_TB_E_SHIFT
assert run(frame(), 0) == abi.TS_TB_E_CHANNELS
assert run(frame(), 4) == abi.TS_TB_E_CHANNELS
assert run(frame(table=0x5000), 3) == abi.TS_TB_E_ORDER, "both channel types in one call with a scale table"
empty = [[0] * (NC + 1), [0] * (NC + 1)]
assert run(frame(n=0, cf=empty)) == 0, "an empty picture is fine"
assert run(frame(n=0, cf=empty, lv=0x4000, levels=0x5000, table=0x6000, size_y=32), 1) == 0
assert run(frame(n=0, cf=empty, table=0x6000), 2) == 0
assert run(frame(n=0, cf=empty, size_y=0)) == 0, "size_y is read with a scale table only"
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    assert b"validated" in r.stdout


def test_grouping_follows_the_order_rule():
    rng = np.random.default_rng(0x5EED7501)
    specs = [ts.random_spec(rng, c, 0, 0, lw, lh) for c in (2, 0, 1) for (lw, lh) in (ts.CHROMA_SHAPES if c else ts.LUMA_SHAPES)]
    sp, cf = ts.group(specs)
    assert cf[0][0] == 0 and cf[0][ts.NC] == cf[1][0] == len(ts.LUMA_SHAPES) and cf[1][ts.NC] == len(sp) == len(specs)
    for ch in range(2):
        for k in range(ts.NC):
            assert cf[ch][k + 1] > cf[ch][k]
            assert all((s["c_idx"] > 0) == ch and ts.area_class(s["lw"], s["lh"]) == k for s in sp[cf[ch][k]:cf[ch][k + 1]])
    assert [ts.area_class(*s) for s in ((1, 2), (2, 2), (1, 5), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5))] == [0, 0, 1, 1, 2, 2, 3, 3]
    assert len(ts.LUMA_SHAPES) == 16 and len(ts.CHROMA_SHAPES) == 24 and (1, 1) not in ts.CHROMA_SHAPES


@pytest.mark.parametrize("vert", [0, 1])
def test_saturating_levels_tell_the_clipped_scan_from_a_prefix_sum(orc, vert):
    """A condition on the inputs, by the oracle alone: on every shape the reference's running sum (clipped after every step) differs from
    numpy.cumsum of the same levels, the levels fit the packed stream, and over each block both ends of the range are reached."""
    hi, lo = (1 << 15) - 1, -(1 << 15)
    for (lw, lh) in ts.CHROMA_SHAPES:
        w, h = 1 << lw, 1 << lh
        c = ts.saturating_levels(w, h, vert)
        assert c.shape == (h, w) and c.min() >= lo and c.max() <= hi
        want = ts.bdpcm(orc, c, vert)
        plain = np.cumsum(c.astype(np.int64), axis=0 if vert else 1)
        assert want.min() == lo and want.max() == hi, (w, h)
        assert np.any(want != plain), (w, h)
        # the oracle's scan is the clipped one, step by step
        ref = c.astype(np.int64).copy()
        for k in range(1, h if vert else w):
            if vert:
                ref[k] = np.clip(ref[k] + ref[k - 1], lo, hi)
            else:
                ref[:, k] = np.clip(ref[:, k] + ref[:, k - 1], lo, hi)
        assert np.array_equal(want, ref), (w, h)
        n = h if vert else w
        if n > 4:                                            # a saturated partial sum is carried from one 4x4 tile into the next
            edge = want[3::4, :][:-1] if vert else want[:, 3::4][:, :-1]
            assert np.any((edge == hi) | (edge == lo)), (w, h)


def test_scaling_of_a_saturated_sum_leaves_the_int16_domain_at_range_20(orc):
    """Why the kernel keeps the full 32-bit scaling arithmetic: at range 20 a running sum reaches -2^20, far outside the |c| < 2^15 domain of
    the 24-bit multiplies; the oracle scales it like any other level."""
    rbits = 20
    c = np.zeros((4, 8), np.int32)
    c[:, :] = -(1 << 18)
    s = ts.spec(0, 0, 0, 3, 2, c, 8, 4, qp=22, bdpcm=True, vert=False)
    summed = ts.bdpcm(orc, c, 0, rbits)
    assert summed.min() == -(1 << rbits)
    res = ts.oracle_residual(orc, s, 12, rbits)
    assert res.min() >= -(1 << rbits) and res.max() < (1 << rbits) and np.any(res != 0)

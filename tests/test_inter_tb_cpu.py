"""CPU: the ABI of vvc355_inter_tb_pass — record and frame layouts as the header declares them, the frame validation, which precedes
every HIP call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot hide), and the
case module's own premises: when the two unit rules of the chroma scale agree, and that the large coding unit case tells them apart."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import inter_tb_cases as tc
from conftest import ROOT
from ffvvc_amd import abi


def test_record_and_frame_layouts_match_the_header():
    assert ctypes.sizeof(abi.InterTu) == 16
    offs = {n: getattr(abi.InterTu, n).offset for n, _ in abi.InterTu._fields_}
    assert offs == dict(coeff_off=0, x0=4, y0=6, log2_w=8, log2_h=9, nzw=10, nzh=11, qp=12, tu_flags=13, flags=14, joint_mts=15)
    assert ctypes.sizeof(abi.InterTbFrame) == 312
    offs = {n: getattr(abi.InterTbFrame, n).offset for n, _ in abi.InterTbFrame._fields_}
    assert offs == dict(tus=0, coeffs=8, lv=16, levels=24, plane=32, scale_table=56, stride=64, width=76, height=80, n_tus=84, hs=88, vs=89,
                        size_y=90, range=91, bd=92, pad_=93, bin_first=96)
    assert abi.BATCH_SIGNATURES["inter_tb_pass"] == ("i", "pppi")
    # the header's own words: field order of both structs, the flag bits and the number of bins
    hdr = open(f"{ROOT}/include/vvc_mi355.h").read()
    for name, cls in (("vvc355_inter_tu", abi.InterTu), ("vvc355_inter_tb_frame", abi.InterTbFrame)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert names == [n for n, _ in cls._fields_], name
    enums = dict(re.findall(r"(VVC355_INTER_T[UB]_\w+) = (-?\d+)", hdr))
    assert {k: int(v) for k, v in enums.items()} == dict(
        VVC355_INTER_TU_DEP_QUANT=abi.INTER_TU_DEP_QUANT, VVC355_INTER_TU_KEEP=abi.INTER_TU_KEEP, VVC355_INTER_TU_UNIT_DX=abi.INTER_TU_UNIT_DX,
        VVC355_INTER_TU_UNIT_DY=abi.INTER_TU_UNIT_DY, VVC355_INTER_TB_BINS=abi.INTER_TB_BINS, VVC355_INTER_TB_E_BINS=abi.INTER_TB_E_BINS,
        VVC355_INTER_TB_E_BD=abi.INTER_TB_E_BD, VVC355_INTER_TB_E_RANGE=abi.INTER_TB_E_RANGE, VVC355_INTER_TB_E_LEVELS=abi.INTER_TB_E_LEVELS,
        VVC355_INTER_TB_E_SIZE_Y=abi.INTER_TB_E_SIZE_Y, VVC355_INTER_TB_E_SHIFT=abi.INTER_TB_E_SHIFT,
        VVC355_INTER_TB_E_CHANNELS=abi.INTER_TB_E_CHANNELS, VVC355_INTER_TB_E_ORDER=abi.INTER_TB_E_ORDER)


def test_error_codes_are_distinct_and_negative():
    codes = [abi.INTER_TB_E_BINS, abi.INTER_TB_E_BD, abi.INTER_TB_E_RANGE, abi.INTER_TB_E_LEVELS, abi.INTER_TB_E_SIZE_Y, abi.INTER_TB_E_SHIFT,
             abi.INTER_TB_E_CHANNELS, abi.INTER_TB_E_ORDER]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_inter_tb_pass.restype = ctypes.c_int
lib.vvc355_inter_tb_pass.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int]
NB = abi.INTER_TB_BINS

def frame(n=52, bins=None, bd=10, rng=15, lv=0, levels=0, table=0, size_y=64, hs=1, vs=1):
    f = abi.InterTbFrame()
    f.tus, f.coeffs, f.lv, f.levels, f.n_tus, f.scale_table = 0x1000, 0x2000, lv, levels, n, table
    for c in range(3):
        f.plane[c], f.stride[c] = 0x10000 * (c + 1), 512
    f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = 256, 128, hs, vs, size_y, rng, bd
    if bins is None:
        bins = list(range(2 * NB + 2))            # one record per bin: 0..26 | 26..52
        bins = [bins[:NB + 1], [v - 1 for v in bins[NB + 1:]]]
    for ch in range(2):
        for k in range(NB + 1):
            f.bin_first[ch][k] = bins[ch][k]
    return f

def run(f, channels=3):
    return lib.vvc355_inter_tb_pass(None, 0x3000, ctypes.addressof(f), channels)

def bins(edit):
    b = [list(range(NB + 1)), list(range(NB, 2 * NB + 1))]
    edit(b)
    return b

def swap(b): b[0][3], b[0][4] = b[0][4], b[0][3]
def gap(b): b[1][0] += 1
def short(b): b[1][NB] -= 1
def first(b): b[0][0] = 1
def chroma_down(b): b[1][7] = b[1][6] - 1

assert run(frame(bins=bins(swap))) == abi.INTER_TB_E_BINS, "luma bins not monotonic"
assert run(frame(bins=bins(chroma_down))) == abi.INTER_TB_E_BINS, "chroma bins not monotonic"
assert run(frame(bins=bins(gap))) == abi.INTER_TB_E_BINS, "chroma does not start where luma ends"
assert run(frame(bins=bins(short))) == abi.INTER_TB_E_BINS, "last bin does not end at n_tus"
assert run(frame(bins=bins(first))) == abi.INTER_TB_E_BINS, "first bin does not start at 0"
assert run(frame(n=-1, bins=[[0] * (NB + 1), [0] * NB + [-1]])) == abi.INTER_TB_E_BINS
assert lib.vvc355_inter_tb_pass(None, 0x3000, None, 3) == abi.INTER_TB_E_BINS, "no host frame"
assert run(frame(bd=9)) == abi.INTER_TB_E_BD
assert run(frame(rng=14)) == abi.INTER_TB_E_RANGE
assert run(frame(rng=21)) == abi.INTER_TB_E_RANGE
assert run(frame(lv=0x4000)) == abi.INTER_TB_E_LEVELS, "lv without levels"
assert run(frame(levels=0x4000)) == abi.INTER_TB_E_LEVELS, "levels without lv"
assert run(frame(table=0x5000, size_y=128), 2) == abi.INTER_TB_E_SIZE_Y
assert run(frame(table=0x5000, size_y=16), 1) == abi.INTER_TB_E_SIZE_Y
assert run(frame(hs=2)) == abi.INTER_TB_E_SHIFT
assert run(frame(vs=2)) == abi.INTER_TB_E_SHIFT
assert run(frame(), 0) == abi.INTER_TB_E_CHANNELS
assert run(frame(), 4) == abi.INTER_TB_E_CHANNELS
assert run(frame(table=0x5000), 3) == abi.INTER_TB_E_ORDER, "both channel types in one call with a scale table"
empty = [[0] * (NB + 1), [0] * (NB + 1)]
assert run(frame(n=0, bins=empty)) == 0, "an empty picture is fine"
assert run(frame(n=0, bins=empty, lv=0x4000, levels=0x5000, table=0x6000, size_y=32), 1) == 0
assert run(frame(n=0, bins=empty, table=0x6000), 2) == 0
assert run(frame(n=0, bins=empty, size_y=0)) == 0, "size_y is read with a scale table only"
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    assert b"validated" in r.stdout


def test_grouping_follows_the_order_rule():
    rng = np.random.default_rng(0x5EED3F01)
    pic = tc.Picture.random(rng, 10, 256, 128)
    specs = tc.tiled_specs(rng, pic, [(4, 4), (3, 5), (6, 6), (2, 2)], [(3, 3), (1, 3), (5, 5), (3, 1)])
    sp, bf = tc.group(specs)
    assert bf[0][0] == 0 and bf[0][tc.NB] == bf[1][0] and bf[1][tc.NB] == len(sp) == len(specs)
    for ch in range(2):
        for k in range(tc.NB):
            assert all((s["c_idx"] > 0) == ch and tc.shape_bin(s["lw"], s["lh"]) == k for s in sp[bf[ch][k]:bf[ch][k + 1]])
    assert bf[1][26] > bf[1][25] and tc.shape_bin(1, 3) == 25 and tc.shape_bin(6, 6) == 24 and tc.shape_bin(2, 3) == 1


@pytest.mark.parametrize("bd", [8, 10])
def test_unit_rules_agree_for_coding_units_up_to_64(orc, bd):
    """Blocks that lie in their coding unit's first unit (every block of a coding unit of at most 64 luma samples does): the walk gives the
    same planes whichever rule picks the unit.  This is when the old path and the new one may be compared."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3F02 + bd)
    pic = tc.Picture.random(rng, bd, 256, 128, lmcs=True)
    specs, _bf = tc.group(tc.tiled_specs(rng, pic, [(4, 4), (3, 3)], [(3, 3), (4, 2), (2, 2)]))
    offs, n = tc.arena_offsets(specs)
    arena = tc.start_arena(specs, offs, n)
    by_cu, _a, table = tc.oracle_walk(orc, pic, specs, offs, arena, "cu")
    by_block, _a, _t = tc.oracle_walk(orc, pic, specs, offs, arena, "block")
    assert sum(1 for s in specs if s["joint"] & 8) > 50 and len(set(table.tolist())) > 1
    for c in range(3):
        assert np.array_equal(by_cu[c], by_block[c])
        assert np.any(by_cu[c] != pic.planes[c])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_large_cu_case_tells_the_unit_rules_apart(orc, bd):
    """CtbSizeY 128 with coding units of 128 luma samples: the table entries are what orc_lmcs_chroma_scale_flat gives at each unit, the
    coding unit's scale differs from the block's own unit's for at least half of the blocks outside the first unit, and the two walks differ."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3F10 + bd)
    pic, specs = tc.large_cu_case(rng, bd)
    specs, _bf = tc.group(specs)
    offs, n = tc.arena_offsets(specs)
    arena = tc.start_arena(specs, offs, n)
    by_cu, _a, table = tc.oracle_walk(orc, pic, specs, offs, arena, "cu")
    by_block, _a, _t = tc.oracle_walk(orc, pic, specs, offs, arena, "block")
    for (cx, cy, _w, _h) in tc.LARGE_CUS:
        assert table[(cy // 64) * pic.ux + cx // 64] == tc.oracle_unit_scale(orc, pic, by_cu[0], cx // 64, cy // 64)
    far, differ = tc.unit_rule_split(pic, specs, table)
    print(f"bd {bd}: {differ} of {far} blocks outside their coding unit's first unit take another scale by the block rule")
    assert far >= 12 and 2 * differ >= far
    assert any(not np.array_equal(by_cu[c], by_block[c]) for c in (1, 2))
    assert np.array_equal(by_cu[0], by_block[0])

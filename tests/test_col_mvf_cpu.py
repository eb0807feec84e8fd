"""CPU: what vvc355_col_mvf_pass is before any HIP call — the layout and the codes as the header states them; the numpy restatement of
mv_compression (H.266 clause 8.5.2.15) of col_mvf_cases pinned to a scalar loop over the whole range, to values worked by hand and to its
idempotence (which is why a parser may run check_mvset on vectors that are compressed already); the two host helpers; the refusal of every
kind of malformed frame with its own code, in the stated order, in a child process with a stream pointer no runtime could use; and the
premises of the DMVR pictures, counted from the oracle's run."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import col_mvf_cases as cm
import inter_frame_cases as ifc
import ref_inter_cases as ic
import ref_lib
from conftest import ROOT
from ffvvc_amd import abi
from test_pic_digest_cpu import SIZES, _header, _members
from test_picture_cpu import _enum

EVERY = np.arange(-(1 << 17), 1 << 17)


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def test_layout_matches_the_header():
    text = _header()
    assert ctypes.sizeof(abi.ColMv) == 16 and "typedef struct vvc355_col_mv { uint32_t w[2][2]; } vvc355_col_mv;    /* 16 bytes" in text
    assert ctypes.sizeof(abi.ColMvfFrame) == 56 and "vvc355_col_mvf_frame {     /* 56 bytes, no implicit padding */" in text
    members = _members(text, "vvc355_col_mvf_frame")
    assert [m[1] for m in members] == [n for n, _ in abi.ColMvfFrame._fields_]
    off = 0
    for ctype, ident, n in members:                 # no implicit padding: every member starts where the one before ends
        field = getattr(abi.ColMvfFrame, ident)
        assert field.offset == off and off % SIZES[ctype] == 0, ident
        assert field.size == SIZES[ctype] * max(n, 1), ident
        off += field.size
    assert off == 56
    offs = {n: getattr(abi.ColMvfFrame, n).offset for n, _ in abi.ColMvfFrame._fields_}
    assert offs == dict(mvf=0, col=8, jobs_luma=16, records=24, width=32, height=36, mvf_stride=40, col_stride=44, n_jobs=48, flags=52, pad_=53)
    assert abi.BATCH_SIGNATURES["col_mvf_pass"] == ("i", "ppp") and abi.BATCH_SIGNATURES["col_mv_unpack"] == ("v", "pppp")
    assert abi.BATCH_SIGNATURES["col_mvf_scatter"] == ("v", "piiipi")
    # declared with the other two things that leave the device per picture
    assert text.index("int vvc355_pic_output_pass(") < text.index("vvc355_col_mvf_frame") < text.index("vvc355_lmcs_filter(")
    # vvc355_picture is not extended
    assert ctypes.sizeof(abi.Picture) == 568


def test_codes_are_the_headers():
    text = _header()
    codes = _enum(text, "VVC355_COL_MVF_E_")
    names = ("FRAME", "SIZE", "STRIDE", "TABLES", "JOBS", "FLAGS", "OVERLAP")
    assert len(codes) == len(names)
    for i, n in enumerate(names):
        assert codes["VVC355_COL_MVF_E_" + n] == getattr(abi, "COL_MVF_E_" + n) == -(i + 1), n
    assert _enum(text, "VVC355_COL_MVF_COMPRESS") == dict(VVC355_COL_MVF_COMPRESS=abi.COL_MVF_COMPRESS) and abi.COL_MVF_COMPRESS == 1
    # the clause and the lines are cited where the entry is stated, and the idempotence is said
    for cite in ("vvc_mvs.c:220-245", "vvc_mvs.c:1016-1022", "vvc_mvs.c:231-232, :241-242", ":1001-1002", "vvc_mvs.c:57-69", "8.5.2.15", "vvc_inter.c:750-762",
                 "idempotent"):
        assert cite in text, cite


# ---------------------------------------------------------------------------------------------------------------- the restatement, pinned

def test_compress_is_the_scalar_loop_on_the_whole_range():
    got = cm.compress(EVERY)
    want = np.array([cm.compress_scalar(int(v)) for v in EVERY])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    small = np.arange(-31, 32)
    assert np.array_equal(cm.compress(small), small)                     # the identity on |v| < 32
    first = EVERY[got != EVERY]                                          # f = 1 rounds nothing off either: the first vectors that change are +-65
    assert int(first[first > 0].min()) == 65 and int(first[first < 0].max()) == -65
    by_hand = {64: 64, 65: 66, 1001: 1008, -1000: -992, 131071: 131072, -131072: -131072}
    for v, c in by_hand.items():
        assert cm.compress_scalar(v) == c == int(cm.compress(np.array([v]))[0]), v
    # what the field must hold: [-2^17, 2^17], so 19 bits signed and not 18
    assert got.min() == -(1 << 17) and got.max() == 1 << 17
    # what is left of a vector: its leading bit and the five below it
    mag = np.abs(got[got != 0])
    low = np.maximum(np.frexp(mag.astype(np.float64))[1] - 6, 0)
    assert ((mag >> low) << low == mag).all()


def test_compress_is_idempotent_on_the_whole_range():
    """check_mvset (vvc_mvs.c:104) compresses what it reads: on entries that are compressed already it changes nothing."""
    once = cm.compress(EVERY)
    assert np.array_equal(cm.compress(once), once)
    assert int((once != EVERY).sum()) > (1 << 17)                        # and it is no identity


# ---------------------------------------------------------------------------------------------------------------- the host helpers

def _unpack(lib, words):
    e = abi.ColMv()
    for l in range(2):
        for k in range(2):
            e.w[l][k] = int(words[l][k])
    mv, ref, pf = ((ctypes.c_int32 * 2) * 2)(), (ctypes.c_int8 * 2)(99, 99), ctypes.c_uint8(99)
    lib.vvc355_col_mv_unpack(ctypes.addressof(e), ctypes.addressof(mv), ctypes.addressof(ref), ctypes.addressof(pf))
    return [[mv[l][k] for k in range(2)] for l in range(2)], [ref[0], ref[1]], pf.value


def test_pack_then_unpack_returns_the_used_fields(lib):
    m = np.zeros((1, 4), ifc.MVF_DT)                # even positions 0 and 2 are read
    for pf in range(4):
        for mv, ref in (([[1 << 17, -(1 << 17)], [-(1 << 17), 1 << 17]], [15, 0]), ([[-1, 0], [131071, -131071]], [0, 15]), ([[12345, -54321], [-7, 8]], [3, 9])):
            m[0, 0]["mv"], m[0, 0]["ref_idx"], m[0, 0]["pred_flag"] = mv, ref, pf
            m[0, 0]["hpel_if_idx"], m[0, 0]["bcw_idx"], m[0, 0]["ciip_flag"], m[0, 0]["pad_"] = 1, 4, 1, (0xAB, 0xCD)
            words = cm.pack(m, False)[0, 0]
            got_mv, got_ref, got_pf = _unpack(lib, words)
            assert got_pf == pf
            for l in range(2):
                used = (pf >> l) & 1
                assert got_mv[l] == (mv[l] if used else [0, 0]) and got_ref[l] == (ref[l] if used else -1), (pf, l)
            if pf == 0:
                assert not words.any()                                  # an intra unit is sixteen zero bytes
            n_mv, n_ref, n_pf = cm.unpack(words)
            assert n_mv.tolist() == got_mv and n_ref.tolist() == got_ref and int(n_pf) == got_pf
    # the entry is a function of what the reference reads: the other fields and the unused list do not show
    a = m.copy()
    a[0, 0]["pred_flag"], a[0, 0]["mv"], a[0, 0]["ref_idx"] = 1, [[5, 6], [7, 8]], [2, 3]
    b = a.copy()
    b[0, 0]["mv"][1], b[0, 0]["ref_idx"][1] = [-999, 999], 11
    b[0, 0]["hpel_if_idx"], b[0, 0]["bcw_idx"], b[0, 0]["ciip_flag"], b[0, 0]["pad_"] = 0, 0, 0, (0, 0)
    b[0, 1] = b[0, 0]                               # an odd position
    assert np.array_equal(cm.pack(a, True), cm.pack(b, True))


@pytest.mark.parametrize("size", [(4, 4), (12, 20), (136, 72)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_scatter_writes_the_three_fields_at_the_even_positions(lib, size):
    width, height = size
    gw, gh = cm.grid(width, height)
    col_stride, min_pu_width = gw + 3, width // 4 + 5
    col = np.full((gh, col_stride, 2, 2), 0xDEADBEEF, np.uint32)
    col[:, :gw] = cm.pack(cm.directed_table(7, width, height), True)
    tab = np.full((height // 4, min_pu_width), 0x5A, np.uint8).repeat(ifc.MVF_DT.itemsize, axis=1).view(ifc.MVF_DT)
    want = tab.copy()
    mv, ref, pf = cm.unpack(col[:, :gw])
    even = want[0::2, 0:(width // 4):2]
    even["mv"], even["ref_idx"], even["pred_flag"] = mv, ref, pf
    assert {int(v) for v in pf.reshape(-1)} == ({0} if gw * gh == 1 else {0, 1, 2, 3})
    before = col.copy()
    lib.vvc355_col_mvf_scatter(col.ctypes.data, col_stride, width, height, tab.ctypes.data, min_pu_width)
    assert np.array_equal(tab.view(np.uint8), want.view(np.uint8)) and np.array_equal(col, before)
    assert (tab["hpel_if_idx"] == 0x5A).all() and (tab["pad_"] == 0x5A).all() and (tab[1::2].view(np.uint8) == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------------- refusals, in a child

CHILD = f"""
import ctypes, sys
sys.path[:0] = [{ROOT!r}, {ROOT + "/tests"!r}]
import col_mvf_cases as cm
from ffvvc_amd import abi
lib = abi.load()
STREAM = 0x5EED0001          # no stream of any runtime: a launch on it would not return
"""


def test_col_mvf_pass_refuses_malformed_frames_before_any_hip_call():
    body = """
def run(f, dev_ptr=0xf000):
    return lib.vvc355_col_mvf_pass(STREAM, dev_ptr, ctypes.addressof(f) if f is not None else None)

def frame(pad=None, **kw):
    f = cm.valid_frame(**kw)
    if pad is not None:
        f.pad_[pad] = 1
    return f

E = lambda n: getattr(abi, "COL_MVF_E_" + n)
JOBS = dict(jobs=0x200000, records=0x300000)
# 1. no frame
assert run(None) == E("FRAME") and run(frame(), dev_ptr=None) == E("FRAME")
# 2. sizes: <= 0, no multiple of 4, beyond 32764
for kw in (dict(width=0), dict(width=-8), dict(height=0), dict(height=-4), dict(width=418), dict(width=417), dict(height=242), dict(height=3),
           dict(width=32768, mvf_stride=8192, col_stride=4096, height=8), dict(height=32768, width=8)):
    assert run(frame(**kw)) == E("SIZE"), kw
# 3. strides and spans
for kw in (dict(mvf_stride=103), dict(mvf_stride=-104), dict(col_stride=51), dict(col_stride=-52), dict(width=420, mvf_stride=105, col_stride=52),
           dict(height=32764, mvf_stride=10925), dict(height=32764, col_stride=32768)):      # 8191 rows of 24-byte, 4096 rows of 16-byte entries: 2 GiB
    assert run(frame(**kw)) == E("STRIDE"), kw
# 4. tables: missing, or not aligned to 8 / 16 bytes
for kw in (dict(mvf=0), dict(col=0), dict(mvf=0x100004), dict(mvf=0x100001), dict(col=0x800008), dict(col=0x800004)):
    assert run(frame(**kw)) == E("TABLES"), kw
# 5. jobs
for kw in (dict(n_jobs=-1), dict(n_jobs=-1, **JOBS), dict(n_jobs=1), dict(n_jobs=5, jobs=0x200000), dict(n_jobs=5, records=0x300000),
           dict(n_jobs=5, jobs=0x200004, records=0x300000), dict(n_jobs=5, jobs=0x200000, records=0x300008)):
    assert run(frame(**kw)) == E("JOBS"), kw
# 6. flags and pad bytes
for kw in (dict(flags=2), dict(flags=3), dict(flags=0x80), dict(pad=0), dict(pad=1), dict(pad=2)):
    assert run(frame(**kw)) == E("FLAGS"), kw
# 7. col overlapping mvf: in place, and by one byte at either end (416x240: 104 x 60 entries of 24 bytes, 52 x 30 of 16)
mvf_span, col_span = 104 * 60 * 24, 52 * 30 * 16
base = 0x100000
for col in (base, base + 16, base + mvf_span - 16, base - col_span + 16):
    assert run(frame(col=col)) == E("OVERLAP"), hex(col)
# the order of the checks is the order of the codes
bad = dict(width=3, mvf_stride=1, mvf=0, n_jobs=-1, flags=2, col=base)
assert run(frame(**bad), dev_ptr=None) == E("FRAME") and run(frame(**bad)) == E("SIZE")
del bad["width"]
assert run(frame(**bad)) == E("STRIDE")
del bad["mvf_stride"]
assert run(frame(**bad)) == E("TABLES")
del bad["mvf"]
assert run(frame(**bad)) == E("JOBS")
del bad["n_jobs"]
assert run(frame(**bad)) == E("FLAGS")
del bad["flags"]
assert run(frame(**bad)) == E("OVERLAP")
assert [E(n) for n in ("FRAME", "SIZE", "STRIDE", "TABLES", "JOBS", "FLAGS", "OVERLAP")] == [-1, -2, -3, -4, -5, -6, -7]
"""
    r = subprocess.run([sys.executable, "-c", CHILD + body + "\nprint('validated')\n"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1500:])
    assert b"validated" in r.stdout


# ---------------------------------------------------------------------------------------------------------------- premises of the DMVR pictures

@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


def test_listed_pictures_are_the_ones_the_reference_pins(orc):
    golden = ic.load_golden()
    assert [ic.picture(n).bd for n in cm.LISTED_DMVR] == [8, 10, 12]
    for name in cm.LISTED_DMVR:
        run = cm.oracle_run(orc, name)
        assert ic.sha(ic.mvf_bytes(run.dmvr)) == golden[name]["dmvr"], f"{name}: the oracle's tab_dmvr_mvf does not hash to the reference's digest"


def test_dmvr_pictures_meet_their_premises(orc):
    starts_x, starts_y, covered = set(), set(), []
    for name in cm.DMVR_PICTURES:
        pic, run = cm.dmvr_picture(name), cm.oracle_run(orc, name)
        points, starts = cm.refined_points(pic, run)
        assert len(points) >= 1, f"{name}: no grid point lies in a DMVR sub-block whose refined vector differs from the table's"
        # such a point shows in the packed entries, compressed or not ... (the refinement is at least 1/16 sample on vectors this small)
        plain, refined = cm.pack(pic.mvf, False), cm.pack(run.dmvr, False)
        assert all((plain[gy, gx] != refined[gy, gx]).any() for gx, gy, _ in points), name
        # ... and the overlay of the oracle's jobs and records on the unrefined table IS the packing of tab_dmvr_mvf
        for do_compress in (False, True):
            assert np.array_equal(cm.overlay(cm.pack(pic.mvf, do_compress), cm.jobs_of(run.jl), run.rec, pic.width, pic.height, do_compress),
                                  cm.pack(run.dmvr, do_compress)), (name, do_compress)
        starts_x |= {s[0] for s in starts}
        starts_y |= {s[1] for s in starts}
        covered.append(len({(gx, gy) for gx, gy, _ in points}))
        n_jobs = cm.jobs_of(run.jl)
        assert any(not j[4] for j in n_jobs) and any(j[4] for j in n_jobs), f"{name}: jobs with and without DMVR"
    assert starts_x == {0, 4} and starts_y == {0, 4}, (starts_x, starts_y)
    # the listed pictures alone never leave the grid: that is what T0 is for
    assert all(cm.refined_points(ic.picture(n), cm.oracle_run(orc, n))[1] == {(0, 0)} for n in cm.LISTED_DMVR)
    # T0's off-grid units cover ONE grid column (row) although they are 8 wide (high)
    t0 = cm.oracle_run(orc, "T0")
    spans = {(x % 8, y % 8, w, h): (len(range((x + 7) // 8, (x + w + 7) // 8)), len(range((y + 7) // 8, (y + h + 7) // 8)))
             for x, y, w, h, d in cm.jobs_of(t0.jl) if d}
    assert spans[(4, 0, 8, 16)] == (1, 2) and spans[(0, 4, 16, 8)] == (2, 1) and spans[(0, 0, 16, 16)] == (2, 2) and spans[(0, 0, 8, 16)] == (1, 2)
    print(f"grid points with refined motion per picture {dict(zip(cm.DMVR_PICTURES, covered))}")


def test_directed_picture_equals_the_reference_where_it_is_built(orc):
    """T0 is not in tests/golden/ref_inter.json: where the reference library is built, its planes and tab_dmvr_mvf are the reference's."""
    ref = ref_lib.load()
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")
    pic = cm.offgrid_picture()
    want, got = ic.run_picture(ref, "ref", pic), cm.oracle_run(orc, "T0")
    lines = ic.plane_differences(pic, want.planes, got.planes) + ic.dmvr_differences(pic, want.dmvr, got.dmvr)
    assert not lines, "\n".join(lines)

"""CPU: the ABI of vvc355_deblock_qp_rec_pass — the frame's layout as the header declares it, the frame validation, which precedes every HIP
call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot hide) — and the premises
of the GPU test's case list (tests/qp_rec_cases.py): what the pictures and sidecars must contain for the parity to mean something, and
that the end-to-end case's deblocked planes depend on the QP tables."""
import ctypes
import subprocess
import sys

import numpy as np

import qp_rec_cases as qc
import bs_rec_cases as rc
from conftest import ROOT
from ffvvc_amd import abi


def test_frame_layout_matches_the_header():
    assert ctypes.sizeof(abi.QpRecFrame) == 104
    offs = {n: getattr(abi.QpRecFrame, n).offset for n, _ in abi.QpRecFrame._fields_}
    assert offs == dict(cu=0, tu=8, ctu_first_cu=16, ctu_first_tu=24, cu_qp=32, tu_qp_c=40, qp_y=48, qp_c=56, n_cu=72, n_tu=76, unit_pitch=80,
                        width=84, height=88, ctb_width=92, ctb_height=96, ctb_log2=100, n_comp=101, pad_=102)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    assert "} vvc355_qp_rec_frame;" in text and "No implicit padding: 104 bytes" in text
    assert abi.BATCH_SIGNATURES["deblock_qp_rec_pass"] == ("i", "ppp")


CODES = ("FRAME", "SIZE", "CTB", "GRID", "PITCH", "COMP", "COUNT", "RECORDS", "SIDECAR", "OUTPUT")


def test_error_codes_are_distinct_negative_and_the_headers():
    codes = [getattr(abi, "QP_REC_E_" + n) for n in CODES]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    for n, c in zip(CODES, codes):
        assert f"VVC355_QP_REC_E_{n} = {c}" in text, n


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_deblock_qp_rec_pass.restype = ctypes.c_int
lib.vvc355_deblock_qp_rec_pass.argtypes = [ctypes.c_void_p] * 3

def frame(**kw):
    f = abi.QpRecFrame()
    f.cu, f.tu, f.ctu_first_cu, f.ctu_first_tu, f.n_cu, f.n_tu = 0x1000, 0x2000, 0x3000, 0x4000, 10, 20
    f.cu_qp, f.tu_qp_c, f.qp_y, f.qp_c[0], f.qp_c[1] = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
    f.width, f.height, f.ctb_log2, f.ctb_width, f.ctb_height, f.unit_pitch, f.n_comp = 328, 200, 6, 6, 4, 82, 3
    for k, v in kw.items():
        if isinstance(v, list):
            getattr(f, k)[v[0]] = v[1]
        else:
            setattr(f, k, v)
    return f

def run(f):
    return lib.vvc355_deblock_qp_rec_pass(None, 0xf000, ctypes.addressof(f))

assert lib.vvc355_deblock_qp_rec_pass(None, 0xf000, None) == abi.QP_REC_E_FRAME, "no host frame"
assert lib.vvc355_deblock_qp_rec_pass(None, None, ctypes.addressof(frame())) == abi.QP_REC_E_FRAME, "no device frame"
for kw in (dict(width=0), dict(width=-8), dict(height=0), dict(width=330), dict(height=202)):
    assert run(frame(**kw)) == abi.QP_REC_E_SIZE, kw
for v in (4, 8):
    assert run(frame(ctb_log2=v)) == abi.QP_REC_E_CTB, v
for kw in (dict(ctb_width=5), dict(ctb_width=7), dict(ctb_height=3), dict(ctb_height=5), dict(ctb_log2=7)):
    assert run(frame(**kw)) == abi.QP_REC_E_GRID, kw
assert run(frame(unit_pitch=81)) == abi.QP_REC_E_PITCH
for v in (0, 2, 4):
    assert run(frame(n_comp=v)) == abi.QP_REC_E_COMP, v
for kw in (dict(n_cu=-1), dict(n_tu=-1)):
    assert run(frame(**kw)) == abi.QP_REC_E_COUNT, kw
for kw in (dict(cu=0), dict(tu=0), dict(ctu_first_cu=0), dict(ctu_first_tu=0), dict(n_comp=1, cu=0), dict(n_comp=1, ctu_first_cu=0)):
    assert run(frame(**kw)) == abi.QP_REC_E_RECORDS, kw
for kw in (dict(cu_qp=0), dict(tu_qp_c=0), dict(n_comp=1, cu_qp=0)):
    assert run(frame(**kw)) == abi.QP_REC_E_SIDECAR, kw
for kw in (dict(qp_y=0), dict(qp_c=[0, 0]), dict(qp_c=[1, 0]), dict(n_comp=1, qp_y=0)):
    assert run(frame(**kw)) == abi.QP_REC_E_OUTPUT, kw
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    assert b"validated" in r.stdout


def _partition(g, recs, keep):
    """Per unit, the origin of the record of recs[keep] that covers it (x0 + 65536 * y0; -1 where none does)."""
    m = np.full((g.th, g.tw), -1, np.int64)
    for r in recs[keep]:
        m[r["y0"] // 4:(int(r["y0"]) + int(r["h"])) // 4, r["x0"] // 4:(int(r["x0"]) + int(r["w"])) // 4] = int(r["x0"]) + 65536 * int(r["y0"])
    return m


def test_the_case_list_holds_what_the_gpu_test_relies_on(orc):
    for i in range(len(rc.CASES)):
        p = qc.picture(orc, i)
        g = p.g
        tree1 = (p.tu["flags"] & 0x80) != 0
        # every record paints, the picture is covered by both kinds, and sidecars are paired with the grouped records
        assert qc.paints(g, p.cu, p.cu_first).all() and qc.paints(g, p.tu, p.tu_first).all(), i
        assert len(p.cu_qp) == len(p.cu) and p.tu_qp_c.shape == (len(p.tu), 2), i
        assert (_partition(g, p.cu, np.ones(len(p.cu), bool)) >= 0).all() and (_partition(g, p.tu, tree1) >= 0).all(), i
        # CTBs where the tree-1 partition is not the tree-0 one: qp_c must come from the tree-1 records
        t0, t1 = _partition(g, p.tu, ~tree1), _partition(g, p.tu, tree1)
        per = 1 << (g.ctb_log2 - 2)
        differ = [np.any(t0[y:y + per, x:x + per] != t1[y:y + per, x:x + per]) for y in range(0, g.th, per) for x in range(0, g.tw, per)]
        assert any(differ), i
        # negative QpY, Cb != Cr for most units, and the value ranges of the issue
        assert p.cu_qp.min() >= -qc.QP_BD_OFFSET and p.cu_qp.max() <= 63 and np.any(p.cu_qp < 0), i
        assert p.tu_qp_c.min() >= 0 and p.tu_qp_c.max() <= 63 + qc.QP_BD_OFFSET, i
        assert np.mean(p.tu_qp_c[tree1, 0] != p.tu_qp_c[tree1, 1]) > 0.9, i
        want = qc.expected(p)
        assert np.any(want["qp_y"] < 0) and np.any(want["qp_c0"] != want["qp_c1"]), i
    # geometry the list must span: CTU 32 / 64 / 128, partial right and bottom CTUs, a width in units that is no multiple of 4
    pics = [qc.picture(orc, i) for i in range(len(rc.CASES))]
    assert min(p.cu_qp.min() for p in pics) == -qc.QP_BD_OFFSET and max(p.cu_qp.max() for p in pics) == 63
    assert max(p.tu_qp_c.max() for p in pics) == 63 + qc.QP_BD_OFFSET
    geoms = [p.g for p in pics]
    assert {g.ctb_log2 for g in geoms} == {5, 6, 7}
    assert any(g.width % (1 << g.ctb_log2) and g.height % (1 << g.ctb_log2) for g in geoms) and any(g.tw % 4 for g in geoms)


def test_directed_pictures_have_the_record_counts_claimed():
    p = qc.directed("one_unit")
    assert len(p.cu) == 1 and len(p.tu) == 2 and p.cu["w"][0] == 128 and set(p.tu["w"]) == {128} and set(p.tu["flags"] & 0x80) == {0, 0x80}
    p = qc.directed("all_4x4")
    assert len(p.cu) == 1024 and len(p.tu) == 2048
    assert np.all((p.tu["flags"][1024:] & 0x80) != 0) and not np.any(p.tu["flags"][:1024] & 0x80)          # tree 1 is the second chunk of 1024
    p = qc.directed("odd_widths")
    tree1 = (p.tu["flags"] & 0x80) != 0
    assert {12, 24, 48} <= set(p.cu["w"]) and {12, 24, 48} <= set(p.tu["w"][tree1])
    for name in qc.DIRECTED:
        p = qc.directed(name)
        assert qc.paints(p.g, p.cu, p.cu_first).all() and qc.paints(p.g, p.tu, p.tu_first).all(), name
        # no two records of a kind and tree overlap: the painted area equals the sum of the rectangles
        tree1 = (p.tu["flags"] & 0x80) != 0
        for recs, keep in ((p.cu, np.ones(len(p.cu), bool)), (p.tu, tree1)):
            area = int(np.sum(recs["w"][keep].astype(int) * recs["h"][keep].astype(int))) // 16
            assert int(np.count_nonzero(_partition(p.g, recs, keep) >= 0)) == area, name
    want = qc.expected(qc.directed("odd_widths"))
    assert all(np.any(want[n] == 0) and np.any(want[n] != 0) for n in qc.TABLES)           # covered and uncovered units in every table


def test_painter_is_the_table_setters_definition():
    """Three records by hand: later records do not matter for units they do not cover, tree 0 never reaches qp_c, values are copied as bytes."""
    p = qc.single_ctu([(0, 0, 8, 4, 0), (8, 0, 4, 8, 0)], [(0, 0, 8, 8, 0x01), (4, 4, 8, 4, 0x80)], 203)
    p.cu_qp[:] = (-12, 63)
    p.tu_qp_c[:] = ((70, 71), (5, 75))
    want = qc.expected(p)
    assert want["qp_y"][0, :4].tolist() == [-12, -12, 63, 0] and want["qp_y"][1, :4].tolist() == [0, 0, 63, 0]
    assert want["qp_c0"][1, :4].tolist() == [0, 5, 5, 0] and want["qp_c1"][1, :4].tolist() == [0, 75, 75, 0]
    assert not want["qp_c0"][0].any() and int(np.count_nonzero(want["qp_c0"])) == 2


def test_end_to_end_case_depends_on_the_qp_tables(orc):
    for i in qc.E2E:
        qp = qc.expected(qc.picture(orc, i))
        planes, _, _ = qc.e2e_inputs(orc, i)
        want = qc.e2e_oracle(orc, i, qp)
        flat = {n: np.full_like(a, int(np.median(a))) for n, a in qp.items()}
        other = qc.e2e_oracle(orc, i, flat)
        changed = sum(int(np.count_nonzero(a != b)) for a, b in zip(planes, want))
        assert changed > 2000, (i, changed)
        for c in range(3):
            assert np.any(want[c] != other[c]), (i, c)

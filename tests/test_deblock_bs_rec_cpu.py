"""CPU: the ABI of vvc355_deblock_bs_rec_pass — the frame's layout as the header declares it, the frame validation, which precedes every HIP
call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot hide) — and the premises
of the GPU test's case list (tests/bs_rec_cases.py), asserted with the oracle: what the pictures must contain for the parity to mean
something at CTU edges, where the kernel reads its P side through a halo."""
import ctypes
import subprocess
import sys

import numpy as np

import bs_rec_cases as rc
from conftest import ROOT
from ffvvc_amd import abi


def test_frame_layout_matches_the_header():
    assert ctypes.sizeof(abi.BsRecFrame) == 208
    offs = {n: getattr(abi.BsRecFrame, n).offset for n, _ in abi.BsRecFrame._fields_}
    assert offs == dict(cu=0, tu=8, ctu_first_cu=16, ctu_first_tu=24, mvf=32, ref_poc=40, slice_idx=48, ctb_to_col_bd=56, ctb_to_row_bd=64,
                        bs=72, max_len_p=120, max_len_q=136, tb_width_c=152, tb_height_c=160, n_cu=168, n_tu=172, unit_pitch=176, mvf_pitch=180,
                        width=184, height=188, ctb_width=192, ctb_height=196, ctb_log2=200, hs=201, vs=202, n_comp=203, lfase=204, lfate=205, pad_=206)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    assert "} vvc355_bs_rec_frame;" in text and "No implicit padding: 208 bytes" in text
    assert abi.BATCH_SIGNATURES["deblock_bs_rec_pass"] == ("i", "ppp")


CODES = ("FRAME", "SIZE", "CTB", "GRID", "PITCH", "COMP", "SHIFT", "COUNT", "RECORDS", "TABLES", "OUTPUT")


def test_error_codes_are_distinct_negative_and_the_headers():
    codes = [getattr(abi, "BS_REC_E_" + n) for n in CODES]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    for n, c in zip(CODES, codes):
        assert f"VVC355_BS_REC_E_{n} = {c}" in text, n


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_deblock_bs_rec_pass.restype = ctypes.c_int
lib.vvc355_deblock_bs_rec_pass.argtypes = [ctypes.c_void_p] * 3

def frame(**kw):
    f = abi.BsRecFrame()
    f.cu, f.tu, f.ctu_first_cu, f.ctu_first_tu, f.n_cu, f.n_tu = 0x1000, 0x2000, 0x3000, 0x4000, 10, 20
    f.mvf, f.ref_poc, f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = 0x5000, 0x6000, 0x7000, 0x8000, 0x9000
    for d in range(2):
        for c in range(3):
            f.bs[d][c] = 0xa000 + 0x100 * (3 * d + c)
        f.max_len_p[d], f.max_len_q[d] = 0xb000 + 0x100 * d, 0xc000 + 0x100 * d
    f.tb_width_c, f.tb_height_c = 0xd000, 0xe000
    f.width, f.height, f.ctb_log2, f.ctb_width, f.ctb_height, f.unit_pitch, f.mvf_pitch = 328, 200, 6, 6, 4, 82, 82
    f.hs, f.vs, f.n_comp, f.lfase, f.lfate = 1, 1, 3, 1, 1
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(f, k)[v[0]][v[1]] = v[2]
        elif isinstance(v, list):
            getattr(f, k)[v[0]] = v[1]
        else:
            setattr(f, k, v)
    return f

def run(f):
    return lib.vvc355_deblock_bs_rec_pass(None, 0xf000, ctypes.addressof(f))

assert lib.vvc355_deblock_bs_rec_pass(None, 0xf000, None) == abi.BS_REC_E_FRAME, "no host frame"
assert lib.vvc355_deblock_bs_rec_pass(None, None, ctypes.addressof(frame())) == abi.BS_REC_E_FRAME, "no device frame"
for kw in (dict(width=0), dict(width=-8), dict(height=0), dict(width=330), dict(height=202)):
    assert run(frame(**kw)) == abi.BS_REC_E_SIZE, kw
for v in (4, 8):
    assert run(frame(ctb_log2=v)) == abi.BS_REC_E_CTB, v
for kw in (dict(ctb_width=5), dict(ctb_width=7), dict(ctb_height=3), dict(ctb_height=5), dict(ctb_log2=7)):
    assert run(frame(**kw)) == abi.BS_REC_E_GRID, kw
for kw in (dict(unit_pitch=81), dict(mvf_pitch=81)):
    assert run(frame(**kw)) == abi.BS_REC_E_PITCH, kw
for v in (0, 2, 4):
    assert run(frame(n_comp=v)) == abi.BS_REC_E_COMP, v
for kw in (dict(hs=2), dict(vs=2)):
    assert run(frame(**kw)) == abi.BS_REC_E_SHIFT, kw
for kw in (dict(n_cu=-1), dict(n_tu=-1)):
    assert run(frame(**kw)) == abi.BS_REC_E_COUNT, kw
for kw in (dict(cu=0), dict(tu=0), dict(ctu_first_cu=0), dict(ctu_first_tu=0)):
    assert run(frame(**kw)) == abi.BS_REC_E_RECORDS, kw
for k in ("mvf", "ref_poc", "slice_idx", "ctb_to_col_bd", "ctb_to_row_bd"):
    assert run(frame(**{{k: 0}})) == abi.BS_REC_E_TABLES, k
for d in range(2):
    for c in range(3):
        assert run(frame(bs=(d, c, 0))) == abi.BS_REC_E_OUTPUT, ("bs", d, c)
    assert run(frame(max_len_p=[d, 0])) == abi.BS_REC_E_OUTPUT, ("max_len_p", d)
    assert run(frame(max_len_q=[d, 0])) == abi.BS_REC_E_OUTPUT, ("max_len_q", d)
    assert run(frame(n_comp=1, bs=(d, 0, 0))) == abi.BS_REC_E_OUTPUT, ("luma only, bs", d)
    assert run(frame(n_comp=1, max_len_q=[d, 0])) == abi.BS_REC_E_OUTPUT, ("luma only, max_len_q", d)
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    assert b"validated" in r.stdout


def _on_ctu_starts(t, want, name):
    """The entries of an output table on the unit columns (vertical edges, "bs1c" / "p1" / "q1") or rows that start a CTU."""
    d = int(name[2]) if name.startswith("bs") else int(name[1])
    idx = rc.ctu_starts(t, d)
    return want[name][:, idx] if d else want[name][idx, :]


def test_the_case_list_holds_what_the_gpu_test_relies_on(orc):
    luma_bs, p1 = set(), set()
    for i in range(1, len(rc.CASES)):
        t, want = rc.case(orc, i)
        luma_bs |= set(np.unique(want["bs00"])) | set(np.unique(want["bs10"]))
        p1 |= set(np.unique(want["p1"]))
        # vertical edges between two CTUs: the P side comes through the left halo
        for name in ("bs10", "bs11", "bs12"):
            assert {1, 2} <= set(np.unique(_on_ctu_starts(t, want, name))), (i, name)
        # sub-block coding units and an independent chroma tree
        cu, tu, _ = t.records()
        assert np.any(cu["flags"] & 3) and np.any(tu["flags"] & 0x80), i
        assert np.any(t.tbw1.astype(int) << t.hs != t.tbw0) or np.any(t.tbx1 != t.tbx0), i
    assert luma_bs == {0, 1, 2} and {1, 2, 3, 5, 7} <= p1
    for i in (2, 5, 6, 7):
        # horizontal edges between two CTUs: the upper halo, with strengths of both kinds and the long filters
        t, want = rc.case(orc, i)
        for name in ("bs00", "bs01", "bs02"):
            assert {1, 2} <= set(np.unique(_on_ctu_starts(t, want, name))), (i, name)
        lens = set(np.unique(_on_ctu_starts(t, want, "p0"))) | set(np.unique(_on_ctu_starts(t, want, "q0")))
        assert {3, 7} <= lens, (i, lens)
    for i in range(2, 7):
        # suppressed slice and tile edges
        t, want = rc.case(orc, i)
        assert np.any(_on_ctu_starts(t, want, "bs10") == 0) or np.any(_on_ctu_starts(t, want, "bs00") == 0), i

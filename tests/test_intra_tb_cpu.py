"""CPU: the ABI of vvc355_intra_tb_pass — record and frame layouts as the header declares them, and the frame validation, which precedes
every HIP call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot hide)."""
import ctypes
import subprocess
import sys

from conftest import ROOT
from ffvvc_amd import abi


def test_record_and_frame_layouts_match_the_header():
    assert ctypes.sizeof(abi.IntraTu) == 16
    offs = {n: getattr(abi.IntraTu, n).offset for n, _ in abi.IntraTu._fields_}
    assert offs == dict(coeff_off=0, log2_w=4, log2_h=5, nzw=6, nzh=7, c_idx=8, qp=9, flags=10, tu_flags=11, mts_idx=12, lfnst_idx=13,
                        pred_mode_intra=14, pad_=15)
    assert ctypes.sizeof(abi.IntraTbFrame) == 64
    offs = {n: getattr(abi.IntraTbFrame, n).offset for n, _ in abi.IntraTbFrame._fields_}
    assert offs == dict(tus=0, coeffs=8, lv=16, levels=24, n_tus=32, class_first=36, range=60, bd=61, launch_mode=62, pad_=63)
    assert abi.BATCH_SIGNATURES["intra_tb_pass"] == ("i", "ppp")


def test_error_codes_are_distinct_and_negative():
    codes = [abi.INTRA_TB_E_CLASS, abi.INTRA_TB_E_BD, abi.INTRA_TB_E_RANGE, abi.INTRA_TB_E_LEVELS, abi.INTRA_TB_E_MODE]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_intra_tb_pass.restype = ctypes.c_int
lib.vvc355_intra_tb_pass.argtypes = [ctypes.c_void_p] * 3

def frame(n=10, cf=(0, 2, 4, 6, 8, 10), bd=10, rng=15, lv=0, levels=0, mode=0):
    f = abi.IntraTbFrame()
    f.tus, f.coeffs, f.lv, f.levels, f.n_tus = 0x1000, 0x2000, lv, levels, n
    for k in range(6):
        f.class_first[k] = cf[k]
    f.range, f.bd, f.launch_mode = rng, bd, mode
    return f

def run(f):
    return lib.vvc355_intra_tb_pass(None, 0x3000, ctypes.addressof(f))

assert run(frame(cf=(0, 4, 2, 6, 8, 10))) == abi.INTRA_TB_E_CLASS, "non-monotonic class_first"
assert run(frame(cf=(0, 2, 4, 6, 8, 9))) == abi.INTRA_TB_E_CLASS, "class_first[5] != n_tus"
assert run(frame(cf=(1, 2, 4, 6, 8, 10))) == abi.INTRA_TB_E_CLASS, "class_first[0] != 0"
assert run(frame(bd=9)) == abi.INTRA_TB_E_BD
assert run(frame(rng=14)) == abi.INTRA_TB_E_RANGE
assert run(frame(rng=21)) == abi.INTRA_TB_E_RANGE
assert run(frame(lv=0x4000)) == abi.INTRA_TB_E_LEVELS, "lv without levels"
assert run(frame(levels=0x4000)) == abi.INTRA_TB_E_LEVELS, "levels without lv"
assert run(frame(mode=3)) == abi.INTRA_TB_E_MODE
assert run(frame(n=0, cf=(0,) * 6)) == 0, "an empty picture is fine"
assert run(frame(n=0, cf=(0,) * 6, lv=0x4000, levels=0x5000, mode=2)) == 0
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-600:])
    assert b"validated" in r.stdout

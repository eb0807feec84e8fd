"""CPU: what vvc355_picture_pass and its pieces do before any HIP call — the layouts as the header states them, vvc355_recon_order_check
(host only) on the orders the RECON case lists produce and on each kind of broken order, the frame validation of vvc355_lmcs_frame_pass,
and the validation of a whole picture: which stage refused it and with which of that stage's own codes.  The validation runs in a child
process with a stream pointer no runtime could use, so that a launch that should not have happened cannot hide."""
import ctypes
import re
import subprocess
import sys

import numpy as np
import pytest

import picture_cases as pcs
from conftest import ROOT
from ffvvc_amd import abi


def _header():
    return open(f"{ROOT}/include/vvc_mi355.h").read()


def test_layouts_match_the_header():
    assert ctypes.sizeof(abi.LmcsFrame) == 64 and ctypes.sizeof(abi.StageRef) == 16 and ctypes.sizeof(abi.Picture) == 568
    offs = {n: getattr(abi.LmcsFrame, n).offset for n, _ in abi.LmcsFrame._fields_}
    assert offs == dict(plane=0, inv_lut=8, slice_idx=16, slice_lmcs_used=24, stride=32, width=36, height=40, ctb_width=44, ctb_height=48,
                        n_slices=52, ctb_log2=56, pad_=57)
    offs = {n: getattr(abi.Picture, n).offset for n, _ in abi.Picture._fields_}
    assert [offs[n] for n in abi.PIC_STAGES] == list(range(0, 16 * 17, 16))
    assert (offs["alf_work"], offs["recon_ctus_host"], offs["recon_order_host"], offs["refs"], offs["done"], offs["n_refs"]) == (272, 280, 288, 296, 552, 560)
    text = _header()
    # the stage pairs in the header's order
    body = re.search(r"typedef struct vvc355_picture \{(.*?)\} vvc355_picture;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"vvc355_stage_ref\s+([^;]+);", body) for n in decl.split(",")]
    assert tuple(names) == abi.PIC_STAGES
    assert "No implicit padding: 568 bytes" in text and "No implicit padding: 64 bytes" in text
    for name, sig in dict(picture_pass=("i", "pip"), lmcs_frame_pass=("i", "pipp"), recon_order_check=("i", "piipi"),
                          inter_frame_predict=("v", "pipp"), affine_frame_predict=("v", "pipp"), gpm_frame_predict=("v", "pipp"),
                          ciip_frame_predict=("i", "pipp")).items():
        assert abi.BATCH_SIGNATURES[name] == sig, name
    for name, sig in dict(event_create=("p", ""), event_destroy=("v", "p"), event_record=("v", "pp"), stream_wait_event=("v", "pp"),
                          event_query=("i", "p")).items():
        assert abi.RUNTIME_SIGNATURES[name] == sig, name


def _enum(text, prefix):
    """{name: value} of the enumerators `prefix`* in the header (explicit values, or counting on from the previous one)."""
    out = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S)):
        value = -1
        for item in body.split(","):
            item = item.strip()
            if not item:
                continue
            name, _, v = item.partition("=")
            try:
                value = int(v.strip(), 0) if v.strip() else value + 1
            except ValueError:          # an expression: none of the enumerators looked at here
                continue
            if name.strip().startswith(prefix):
                out[name.strip()] = value
    return out


def test_codes_and_stage_ids_are_the_headers_and_fit_eight_bits():
    text = _header()
    stages = _enum(text, "VVC355_PIC_STAGE_")
    assert stages["VVC355_PIC_STAGE_PICTURE"] == abi.PIC_STAGE_PICTURE == 1 and stages["VVC355_PIC_STAGE_RECON_ORDER"] == abi.PIC_STAGE_RECON_ORDER
    for n in abi.PIC_STAGES:
        assert stages["VVC355_PIC_STAGE_" + n.upper()] == pcs.STAGE_ID[n], n
    assert len(set(stages.values())) == len(stages) == len(abi.PIC_STAGES) + 2
    for prefix, names in (("LMCS_FRAME_E_", ("FRAME", "BD", "SIZE", "CTB", "GRID", "STRIDE", "COUNT", "TABLES")),
                          ("RECON_ORDER_E_", ("ARGS", "RANGE", "EMPTY", "DUPLICATE", "MISSING", "DEPENDENCY")),
                          ("PIC_E_", ("NO_DEVICE_FRAME", "PICTURE", "CIIP_CMDS", "SCALE_TABLE", "REFS", "CAPTURE"))):
        codes = _enum(text, "VVC355_" + prefix)
        assert len(codes) == len(names) and len(set(codes.values())) == len(names)
        for n in names:
            assert codes["VVC355_" + prefix + n] == getattr(abi, prefix + n) < 0, n
    # every code of every stage that returns one fits the low 8 bits of the picture's return value, and the macros say what abi.py says
    every = _enum(text, "VVC355_")
    stage_codes = {n: v for n, v in every.items() if re.match(r"VVC355_(INTRA_TB|INTER_TB|TS_TB|CIIP|BS_REC|QP_REC|LMCS_FRAME|RECON_ORDER|PIC)_E_", n)}
    assert len(stage_codes) > 60 and all(-255 <= v < 0 for v in stage_codes.values())
    for name in pcs.CODES:
        assert every["VVC355_" + name] == pcs.CODES[name]
    assert "#define VVC355_PIC_ERROR(stage, code) (-(((stage) << 8) | -(code)))" in text
    assert "#define VVC355_PIC_STAGE(ret)         ((-(ret)) >> 8)" in text and "#define VVC355_PIC_CODE(ret)          (-((-(ret)) & 255))" in text
    assert pcs.decode(-((7 << 8) | 11)) == (7, -11)


# ---------------------------------------------------------------------------------------------------------------- vvc355_recon_order_check

@pytest.fixture(scope="module")
def tables():
    return pcs.recon_tables()


def test_order_check_accepts_the_critical_path_order_and_raster_order(tables):
    import recon_cases
    lib = abi.load()
    light = 0
    for name, ctus, ncx, ncy in tables:
        raster = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
        critical = recon_cases.critical_order(lib, ctus, ncx, ncy)
        assert len(raster) > 3, name
        assert pcs.order_check(lib, ctus, ncx, ncy, raster) == 0, name
        assert pcs.order_check(lib, ctus, ncx, ncy, critical) == 0, name
        light += int((ctus["flags"] & abi.RECON_CTU_LIGHT).any())
    assert light
    # nothing to do is an order too
    empty = np.zeros(6, recon_cases.CTU)
    assert pcs.order_check(lib, empty, 3, 2, np.zeros(0, np.int32)) == 0


def test_order_check_names_each_kind_of_defect(tables):
    lib = abi.load()
    seen = set()
    for name, ctus, ncx, ncy in tables:
        raster = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
        at = {int(rs): i for i, rs in enumerate(raster)}
        # a CTU ahead of one it waits for: swap the pair (every kind of wait the table has: left, upper-left, upper, upper-right, LIGHT's luma waits)
        swaps = 0
        for rs in raster:
            for d in pcs.waits_for(ctus, ncx, rs):
                bad = raster.copy()
                bad[at[int(rs)]], bad[at[d]] = d, rs
                assert pcs.order_check(lib, ctus, ncx, ncy, bad) == abi.RECON_ORDER_E_DEPENDENCY, (name, int(rs), d)
                swaps += 1
                seen.add(int(rs) - d)
        assert swaps, name
        # a LIGHT CTU waits for nothing but the luma it names: moving it in front of its other neighbours is fine
        assert pcs.order_check(lib, ctus, ncx, ncy, np.concatenate([raster[:1], raster[:1], raster[2:]])) == abi.RECON_ORDER_E_DUPLICATE, name
        assert pcs.order_check(lib, ctus, ncx, ncy, raster[:-1]) == abi.RECON_ORDER_E_MISSING, name
        assert pcs.order_check(lib, ctus, ncx, ncy, np.concatenate([raster[:2], raster[3:]])) == abi.RECON_ORDER_E_MISSING, name
        idle = np.nonzero(ctus["n_cmd"] == 0)[0]
        if len(idle):
            assert pcs.order_check(lib, ctus, ncx, ncy, np.concatenate([raster, idle[:1].astype(np.int32)])) == abi.RECON_ORDER_E_EMPTY, name
            seen.add("idle")
        for out_of_range in (-1, ncx * ncy, 1 << 30):
            assert pcs.order_check(lib, ctus, ncx, ncy, np.concatenate([raster[:-1], [out_of_range]])) == abi.RECON_ORDER_E_RANGE, name
    assert {1, "idle"} <= seen and len([s for s in seen if s != "idle"]) >= 4          # left, upper-left, upper, upper-right
    name, ctus, ncx, ncy = tables[0]
    order = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
    table = np.ascontiguousarray(ctus)
    assert lib.vvc355_recon_order_check(None, ncx, ncy, order.ctypes.data, len(order)) == abi.RECON_ORDER_E_ARGS
    assert lib.vvc355_recon_order_check(table.ctypes.data, ncx, ncy, None, len(order)) == abi.RECON_ORDER_E_ARGS
    assert lib.vvc355_recon_order_check(table.ctypes.data, ncx, ncy, order.ctypes.data, -1) == abi.RECON_ORDER_E_ARGS
    assert lib.vvc355_recon_order_check(table.ctypes.data, -1, ncy, order.ctypes.data, len(order)) == abi.RECON_ORDER_E_ARGS


def test_a_light_ctu_may_precede_the_neighbours_it_does_not_name():
    """3 x 2 CTUs, all with commands; CTU 4 (middle of the second row) is LIGHT and waits for the luma of its upper neighbour only: it may
    take its ticket before its left neighbour, an ordinary CTU in its place may not."""
    import recon_cases
    lib = abi.load()
    ctus = np.zeros(6, recon_cases.CTU)
    ctus["n_cmd"] = 10
    ctus[4]["flags"] = abi.RECON_CTU_LIGHT | abi.RECON_CTU_LUMA_UP
    order = [0, 1, 2, 4, 3, 5]
    assert pcs.order_check(lib, ctus, 3, 2, order) == 0
    assert pcs.order_check(lib, ctus, 3, 2, [0, 4, 1, 2, 3, 5]) == abi.RECON_ORDER_E_DEPENDENCY
    ctus[4]["flags"] = 0
    assert pcs.order_check(lib, ctus, 3, 2, order) == abi.RECON_ORDER_E_DEPENDENCY


def test_recon_order_is_unchanged():
    """The checker shares recon_deps() with vvc355_recon_order: the order itself is still the plain restatement of its rule."""
    import recon_cases
    import test_recon_order_cpu as ro
    lib = abi.load()
    ctus = ro.table(np.random.default_rng(0x5EED0EA0 + 12), 12, 7, 0.4, 0.3)
    assert recon_cases.critical_order(lib, ctus, 12, 7).tolist() == ro.restated(ctus, 12, 7)


# ---------------------------------------------------------------------------------------------------------------- validation, in a child

CHILD = f"""
import ctypes, sys
sys.path[:0] = [{ROOT!r}, {ROOT + "/tests"!r}]
import numpy as np
import picture_cases as pcs
from ffvvc_amd import abi
lib = abi.load()
STREAM = 0x5EED0001          # no stream of any runtime: a launch on it would not return
"""


def _child(body):
    r = subprocess.run([sys.executable, "-c", CHILD + body + "\nprint('validated')\n"], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-1200:])
    assert b"validated" in r.stdout


def test_lmcs_frame_pass_refuses_malformed_frames_before_any_hip_call():
    _child("""
def frame(**kw):
    f = pcs.valid_frames()["lmcs"]
    for k, v in kw.items():
        setattr(f, k, v)
    return f

def run(f, bd=10, dev_ptr=0xf000):
    return lib.vvc355_lmcs_frame_pass(STREAM, bd, dev_ptr, ctypes.addressof(f) if f is not None else None)

assert run(None) == abi.LMCS_FRAME_E_FRAME and run(frame(), dev_ptr=None) == abi.LMCS_FRAME_E_FRAME
for bd in (0, 9, 11, 16):
    assert run(frame(), bd) == abi.LMCS_FRAME_E_BD, bd
for kw in (dict(width=0), dict(width=-8), dict(height=0), dict(height=-1), dict(width=1 << 16), dict(height=1 << 16)):
    assert run(frame(**kw)) == abi.LMCS_FRAME_E_SIZE, kw
for v in (0, 4, 8):
    assert run(frame(ctb_log2=v)) == abi.LMCS_FRAME_E_CTB, v
# a geometry that disagrees with ctb_log2
for kw in (dict(ctb_width=5), dict(ctb_width=7), dict(ctb_height=3), dict(ctb_height=5), dict(ctb_log2=5), dict(ctb_log2=7), dict(ctb_width=0)):
    assert run(frame(**kw)) == abi.LMCS_FRAME_E_GRID, kw
# a stride smaller than a row, or no multiple of the pixel size
for kw in (dict(stride=655), dict(stride=0), dict(stride=-1024), dict(stride=657), dict(stride=1 << 23), dict(stride=1 << 22, height=512, ctb_height=8)):
    assert run(frame(**kw)) == abi.LMCS_FRAME_E_STRIDE, kw
assert run(frame(stride=327), 8) == abi.LMCS_FRAME_E_STRIDE
assert run(frame(n_slices=-1)) == abi.LMCS_FRAME_E_COUNT
for name in ("plane", "inv_lut", "slice_idx", "slice_lmcs_used"):
    assert run(frame(**{name: 0})) == abi.LMCS_FRAME_E_TABLES, name
codes = [getattr(abi, "LMCS_FRAME_E_" + n) for n in ("FRAME", "BD", "SIZE", "CTB", "GRID", "STRIDE", "COUNT", "TABLES")]
assert len(set(codes)) == 8 and all(c < 0 for c in codes)
""")


def test_an_empty_picture_returns_zero_without_any_hip_call():
    _child("""
assert pcs.run(lib, STREAM, 10, pcs.picture()) == 0
assert pcs.run(lib, STREAM, 8, abi.Picture()) == 0
assert pcs.decode(lib.vvc355_picture_pass(STREAM, 10, None)) == (abi.PIC_STAGE_PICTURE, abi.PIC_E_PICTURE)
# stages whose records are empty pass the validation and have nothing to launch
f = pcs.valid_frames()
f["ciip"].n_cus = 0
for n in ("intra_tb", "inter_tb", "ts_tb"):
    f[n].n_tus = 0
for k in range(6):
    f["intra_tb"].class_first[k] = 0
for ch in range(2):
    for k in range(abi.INTER_TB_BINS + 1):
        f["inter_tb"].bin_first[ch][k] = 0
    for k in range(abi.TS_TB_CLASSES + 1):
        f["ts_tb"].class_first[ch][k] = 0
assert pcs.run(lib, STREAM, 10, pcs.picture({n: (0xf000, f[n]) for n in ("ciip", "intra_tb", "inter_tb", "ts_tb")})) == 0
""")


def test_a_malformed_stage_is_named_with_its_own_code_and_nothing_is_launched():
    _child("""
def setpath(obj, path, v):
    setattr(obj, path, v)

assert len({m[0] for m in pcs.MALFORMED}) == len(pcs.MALFORMED) == 7
for (stage, field, value, code) in pcs.MALFORMED:
    f = pcs.valid_frames()
    setpath(f[stage], field, value)
    # the stage's own entry says the same (it launches nothing either)
    entry = dict(ciip=lambda: lib.vvc355_ciip_frame_pass(STREAM, 10, 0xf000, ctypes.addressof(f["ciip"])),
                 intra_tb=lambda: lib.vvc355_intra_tb_pass(STREAM, 0xf000, ctypes.addressof(f["intra_tb"])),
                 inter_tb=lambda: lib.vvc355_inter_tb_pass(STREAM, 0xf000, ctypes.addressof(f["inter_tb"]), 3),
                 ts_tb=lambda: lib.vvc355_ts_tb_pass(STREAM, 0xf000, ctypes.addressof(f["ts_tb"]), 3),
                 bs_rec=lambda: lib.vvc355_deblock_bs_rec_pass(STREAM, 0xf000, ctypes.addressof(f["bs_rec"])),
                 qp_rec=lambda: lib.vvc355_deblock_qp_rec_pass(STREAM, 0xf000, ctypes.addressof(f["qp_rec"])),
                 lmcs=lambda: lib.vvc355_lmcs_frame_pass(STREAM, 10, 0xf000, ctypes.addressof(f["lmcs"])))[stage]
    assert entry() == pcs.code_of(code), (stage, entry())
    # every checked stage present and valid but this one; alone; and as the last stage of the order with unchecked stages in front
    for others in (list(f), [stage]):
        pic = pcs.picture({n: (0xf000, f[n]) for n in others})
        got = pcs.decode(pcs.run(lib, STREAM, 10, pic))
        assert got == (pcs.STAGE_ID[stage], pcs.code_of(code)), (stage, others, got)
# the bit depth is the picture's: the CIIP and LMCS stages compare it with their frames
f = pcs.valid_frames()
assert pcs.decode(pcs.run(lib, STREAM, 8, pcs.picture({n: (0xf000, f[n]) for n in f}))) == (abi.PIC_STAGE_CIIP, abi.CIIP_E_DEPTH)
assert pcs.decode(pcs.run(lib, STREAM, 9, pcs.picture(dict(lmcs=(0xf000, f["lmcs"]))))) == (abi.PIC_STAGE_LMCS, abi.LMCS_FRAME_E_BD)
# a stage given without its device descriptor, checked stage or not; the ALF stage also needs its work buffer
for n in abi.PIC_STAGES:
    frame = f.get(n, abi.SaoFrame())
    assert pcs.decode(pcs.run(lib, STREAM, 10, pcs.picture({n: (0, frame)}))) == (pcs.STAGE_ID[n], abi.PIC_E_NO_DEVICE_FRAME), n
assert pcs.decode(pcs.run(lib, STREAM, 10, pcs.picture(dict(alf=(0xf000, abi.AlfFrame()))))) == (abi.PIC_STAGE_ALF, abi.PIC_E_NO_DEVICE_FRAME)
# a broken ticket order, through the picture: the recon frame gives the grid and n_work
import recon_cases
ctus = np.zeros(6, recon_cases.CTU)
ctus["n_cmd"] = 10
rf = abi.ReconFrame()
rf.ctb_width, rf.ctb_height, rf.n_work = 3, 2, 6
for order, code in (([0, 1, 2, 3, 4, 5], None), ([0, 1, 2, 4, 3, 5], abi.RECON_ORDER_E_DEPENDENCY), ([0, 1, 2, 3, 4, 4], abi.RECON_ORDER_E_DUPLICATE),
                    ([0, 1, 2, 3, 4, 6], abi.RECON_ORDER_E_RANGE)):
    if code is None:
        continue                    # a picture that passes would launch the pass
    pic = pcs.picture(dict(recon=(0xf000, rf)), recon_tables=(ctus, np.array(order, np.int32)))
    assert pcs.decode(pcs.run(lib, STREAM, 10, pic)) == (abi.PIC_STAGE_RECON_ORDER, code), order
rf.n_work = 5
pic = pcs.picture(dict(recon=(0xf000, rf)), recon_tables=(ctus, np.array([0, 1, 2, 3, 4, 5], np.int32)))
assert pcs.decode(pcs.run(lib, STREAM, 10, pic)) == (abi.PIC_STAGE_RECON_ORDER, abi.RECON_ORDER_E_MISSING)
ctus[5]["n_cmd"] = 0
pic = pcs.picture(dict(recon=(0xf000, rf)), recon_tables=(ctus, np.array([0, 1, 2, 3, 5], np.int32)))
assert pcs.decode(pcs.run(lib, STREAM, 10, pic)) == (abi.PIC_STAGE_RECON_ORDER, abi.RECON_ORDER_E_EMPTY)
""")


def test_each_cross_check_of_the_picture_is_refused():
    _child("""
def refused(pic, code, bd=10):
    got = pcs.decode(pcs.run(lib, STREAM, bd, pic))
    assert got == (abi.PIC_STAGE_PICTURE, code), got

f = pcs.valid_frames()
# ciip.cmds, when set, is recon.cmds
f["ciip"].cmds = 0xb000
rf = abi.ReconFrame()
rf.cmds = f["ciip"].cmds + 64
refused(pcs.picture(dict(ciip=(0xf000, f["ciip"]), recon=(0xf100, rf))), abi.PIC_E_CIIP_CMDS)
refused(pcs.picture(dict(ciip=(0xf000, f["ciip"]))), abi.PIC_E_CIIP_CMDS)               # commands patched for a walk that is not there
# a scale table of a TB pass is lmcs_scale.scale, and that stage is present
sf = abi.LmcsScaleFrame()
sf.scale, sf.size_y = 0x77000, 64
for name in ("inter_tb", "ts_tb"):
    g = pcs.valid_frames()
    g[name].scale_table = 0x77000
    refused(pcs.picture({name: (0xf000, g[name])}), abi.PIC_E_SCALE_TABLE)
    g[name].scale_table = 0x77040
    refused(pcs.picture({name: (0xf000, g[name]), "lmcs_scale": (0xf100, sf)}), abi.PIC_E_SCALE_TABLE)
# references: at most 32, none of them null
pic = pcs.picture(refs=[0x1000] * 3)
pic.n_refs = 33
refused(pic, abi.PIC_E_REFS)
pic.n_refs = -1
refused(pic, abi.PIC_E_REFS)
refused(pcs.picture(refs=[0x1000, 0, 0x3000]), abi.PIC_E_REFS)
# ... and all of it before any stage check: a malformed stage does not hide it, nor the other way round once the rule is met
g = pcs.valid_frames()
g["lmcs"].stride = 1
refused(pcs.picture(dict(lmcs=(0xf000, g["lmcs"])), refs=[0]), abi.PIC_E_REFS)
""")

"""CPU: the ABI of vvc355_ciip_frame_build / _pass — the record's and the frame's layout as the header states them, the frame validation,
which precedes every HIP call and therefore runs without a GPU (in a child process, so that a launch that should not have happened cannot
hide) — and the premises of the GPU test's case list (tests/ciip_frame_cases.py): what the pictures must contain for the parity to mean
something."""
import ctypes
import subprocess
import sys

import numpy as np

import ciip_frame_cases as cc
from conftest import ROOT
from ffvvc_amd import abi


def test_layouts_match_the_header():
    assert ctypes.sizeof(abi.CiipCu) == 32 and ctypes.sizeof(abi.CiipFrame) == 224
    offs = {n: getattr(abi.CiipCu, n).offset for n, _ in abi.CiipCu._fields_}
    assert offs == dict(x0=0, y0=2, cb_width=4, cb_height=6, hpel_if_idx=8, slice=9, pad_=10, first_job=12, scratch_off=16, cmd=20)
    offs = {n: getattr(abi.CiipFrame, n).offset for n, _ in abi.CiipFrame._fields_}
    assert offs == dict(pic=0, cus=136, jobs=144, scratch=152, cmds=160, slice_idx=168, ctb_to_col_bd=176, ctb_to_row_bd=184, n_cus=192, n_jobs=196,
                        scratch_len=200, n_slices=204, n_cmds=208, ctb_width=212, ctb_height=216, ctb_log2=220, pad_=221)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    assert "} vvc355_ciip_cu;" in text and "} vvc355_ciip_frame;" in text
    assert "No implicit padding: vvc355_ciip_cu 32 bytes, vvc355_ciip_frame 224 bytes" in text
    assert abi.BATCH_SIGNATURES["ciip_frame_build"] == ("i", "ppp") and abi.BATCH_SIGNATURES["ciip_frame_pass"] == ("i", "pipp")


CODES = ("FRAME", "SIZE", "CTB", "GRID", "COUNT", "DEPTH", "FORMAT", "RECORDS", "JOBS", "TABLES", "CMDS")


def test_error_codes_are_distinct_negative_and_the_headers():
    codes = [getattr(abi, "CIIP_E_" + n) for n in CODES]
    assert all(c < 0 for c in codes) and len(set(codes)) == len(codes)
    text = open(f"{ROOT}/include/vvc_mi355.h").read()
    for n, c in zip(CODES, codes):
        assert f"VVC355_CIIP_E_{n} = {c}" in text, n


def test_bad_frames_are_refused_before_any_hip_call():
    code = f"""
import ctypes, sys
sys.path.insert(0, {ROOT!r})
from ffvvc_amd import abi
lib = ctypes.CDLL(abi.LIB_PATH)
lib.vvc355_ciip_frame_pass.restype = lib.vvc355_ciip_frame_build.restype = ctypes.c_int
lib.vvc355_ciip_frame_pass.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
lib.vvc355_ciip_frame_build.argtypes = [ctypes.c_void_p] * 3

def frame(**kw):
    f = abi.CiipFrame()
    p = f.pic
    p.dst[0], p.dst[1], p.dst[2], p.mvf, p.refs, p.slices, p.lmcs_fwd_lut = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
    p.dst_stride[0], p.dst_stride[1], p.dst_stride[2], p.mvf_stride = 1024, 512, 512, 82
    p.width, p.height, p.hs, p.vs, p.chroma_format_idc, p.pixel_shift = 328, 200, 1, 1, 1, 1
    f.cus, f.jobs, f.scratch, f.cmds, f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = 0x8000, 0x9000, 0xa000, 0xb000, 0xc000, 0xd000, 0xe000
    f.n_cus, f.n_jobs, f.scratch_len, f.n_slices, f.n_cmds, f.ctb_width, f.ctb_height, f.ctb_log2 = 10, 60, 4096, 2, 40, 6, 4, 6
    for k, v in kw.items():
        tgt, k = (f.pic, k[4:]) if k.startswith("pic_") else (f, k)
        if isinstance(v, list):
            getattr(tgt, k)[v[0]] = v[1]
        else:
            setattr(tgt, k, v)
    return f

def run(f, bd=10):
    a = lib.vvc355_ciip_frame_pass(None, bd, 0xf000, ctypes.addressof(f))
    b = lib.vvc355_ciip_frame_build(None, 0xf000, ctypes.addressof(f))
    return a, b

def both(code):
    return (code, code)

assert lib.vvc355_ciip_frame_pass(None, 10, 0xf000, None) == abi.CIIP_E_FRAME, "no host frame"
assert lib.vvc355_ciip_frame_build(None, 0xf000, None) == abi.CIIP_E_FRAME, "no host frame"
assert lib.vvc355_ciip_frame_pass(None, 10, None, ctypes.addressof(frame())) == abi.CIIP_E_FRAME, "no device frame"
assert lib.vvc355_ciip_frame_build(None, None, ctypes.addressof(frame())) == abi.CIIP_E_FRAME, "no device frame"
for kw in (dict(pic_width=0), dict(pic_width=-8), dict(pic_height=0), dict(pic_width=330), dict(pic_height=202)):
    assert run(frame(**kw)) == both(abi.CIIP_E_SIZE), kw
for v in (4, 8):
    assert run(frame(ctb_log2=v)) == both(abi.CIIP_E_CTB), v
for kw in (dict(ctb_width=5), dict(ctb_width=7), dict(ctb_height=3), dict(ctb_height=5), dict(ctb_log2=7)):
    assert run(frame(**kw)) == both(abi.CIIP_E_GRID), kw
for kw in (dict(n_cus=-1), dict(n_jobs=-1), dict(scratch_len=-1), dict(n_slices=-1), dict(n_cmds=-1)):
    assert run(frame(**kw)) == both(abi.CIIP_E_COUNT), kw
# the bit depth is the pass's argument: the build entry has none to compare pixel_shift with
# (no records here: a frame the build entry accepts must not reach a launch on a machine without a GPU)
assert run(frame(n_cus=0), bd=8) == (abi.CIIP_E_DEPTH, 0)
assert run(frame(n_cus=0, pic_pixel_shift=0)) == (abi.CIIP_E_DEPTH, 0)
assert run(frame(n_cus=0, pic_pixel_shift=0), bd=12) == (abi.CIIP_E_DEPTH, 0)
assert run(frame(n_cus=0), bd=9) == (abi.CIIP_E_DEPTH, 0)
assert run(frame(pic_pixel_shift=2)) == both(abi.CIIP_E_DEPTH)
for kw in (dict(pic_hs=2), dict(pic_vs=2), dict(pic_hs=0), dict(pic_vs=0), dict(pic_chroma_format_idc=0), dict(pic_chroma_format_idc=2),
           dict(pic_chroma_format_idc=3), dict(pic_chroma_format_idc=4), dict(pic_chroma_format_idc=2, pic_vs=0, pic_hs=0)):
    assert run(frame(**kw)) == both(abi.CIIP_E_FORMAT), kw
for kw in (dict(pic_chroma_format_idc=2, pic_vs=0), dict(pic_chroma_format_idc=3, pic_vs=0, pic_hs=0), dict(pic_chroma_format_idc=0, pic_vs=0, pic_hs=0, pic_dst=[1, 0])):
    assert run(frame(n_cus=0, **kw)) == both(0), kw
assert run(frame(cus=0)) == both(abi.CIIP_E_RECORDS)
assert run(frame(jobs=0)) == both(abi.CIIP_E_JOBS)
for kw in (dict(scratch=0), dict(pic_mvf=0), dict(pic_refs=0), dict(pic_slices=0), dict(pic_dst=[0, 0]), dict(pic_dst=[1, 0]), dict(pic_dst=[2, 0]), dict(pic_mvf_stride=81)):
    assert run(frame(**kw)) == both(abi.CIIP_E_TABLES), kw
for kw in (dict(slice_idx=0), dict(ctb_to_col_bd=0), dict(ctb_to_row_bd=0)):
    assert run(frame(**kw)) == both(abi.CIIP_E_CMDS), kw
# nothing to do: no records (the other arrays may then be absent), or no job slots
for kw in (dict(n_cus=0), dict(n_cus=0, cus=0), dict(n_cus=0, n_jobs=0, jobs=0), dict(n_jobs=0), dict(n_cus=0, cmds=0, slice_idx=0, ctb_to_col_bd=0, ctb_to_row_bd=0)):
    assert run(frame(**kw)) == both(0), kw
print("validated")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    assert b"validated" in r.stdout


def _unavailable_intra(p):
    """Per unit: which reasons keep an INTRA neighbour from counting (slice above, tile left, tile above), and the picture-edge units."""
    out = dict(slice_above=0, tile_left=0, tile_above=0, picture_top=0, picture_left=0)
    ctb = 1 << p.ctb_log2
    for cu in p.cus:
        x0, y0, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
        rx, ry = x0 >> p.ctb_log2, y0 >> p.ctb_log2
        rs = ry * p.ncx + rx
        out["picture_top"] += y0 == 0
        out["picture_left"] += x0 == 0
        if y0 % ctb == 0 and ry > 0 and p.mvf[(y0 - 1) >> 2, (x0 + w - 1) >> 2]["pred_flag"] == 0:
            same_tile = p.row_bd[ry] == p.row_bd[ry - 1]
            out["tile_above"] += not same_tile
            out["slice_above"] += bool(same_tile and p.slice_idx[rs] != p.slice_idx[rs - p.ncx])
        if x0 % ctb == 0 and rx > 0 and p.mvf[(y0 + h - 1) >> 2, (x0 - 1) >> 2]["pred_flag"] == 0:
            out["tile_left"] += bool(p.col_bd[rx] != p.col_bd[rx - 1])
    return out


def _check_picture(i, p):
    """What every picture of the list must hold; returns its unit sizes and its counts of unavailable intra neighbours."""
    assert all(cc.unit_ok(p, cu) for cu in p.cus), i
    assert p.n_jobs == sum(cc.n_tiles(int(cu["cb_width"]), int(cu["cb_height"]), p.hs, p.vs, p.chroma) for cu in p.cus), i
    w = cc.unit_weights(p)
    assert set(w.tolist()) == {1, 2, 3}, (i, np.bincount(w))
    # units touching the right and the bottom picture edge
    assert np.any(p.cus["x0"] + p.cus["cb_width"] == p.width) and np.any(p.cus["y0"] + p.cus["cb_height"] == p.height), i
    found = _unavailable_intra(p)
    sizes = {(int(cu["cb_width"]), int(cu["cb_height"])) for cu in p.cus}
    if cc.CASES[i][5]:
        assert all(v > 0 for v in found.values()), found               # the picture with tiles: every reason occurs
    # the jobs: uni L0, uni L1, bi; explicit weights; a bi-predicted job with bcw_idx != 0 and nevertheless default weights
    jobs = cc.expect_jobs(p, lambda c: (1 << 40, 4096), lambda l, r, c: ((2 + l) << 40 | r << 32, 4096), 5 << 40, 6 << 40)
    assert np.all(jobs["w"] > 0) and set(np.unique(jobs["pred_flag"])) == {1, 2, 3}, i
    bi = jobs["pred_flag"] == 3
    assert (bi & (jobs["weight_flag"] == 1) & (jobs["denom"] == 6)).any() and (~bi & (jobs["weight_flag"] == 1)).any(), i
    assert not np.isin(jobs["denom"], [2]).any(), i                                        # no bcw weights, ever
    bcw_units = [cu for cu in p.cus if p.mvf[int(cu["y0"]) >> 2, int(cu["x0"]) >> 2]["bcw_idx"] and p.mvf[int(cu["y0"]) >> 2, int(cu["x0"]) >> 2]["pred_flag"] == 3]
    assert bcw_units and all(jobs[int(cu["first_job"])]["weight_flag"] == 0 for cu in bcw_units), i
    assert any(int(cu["slice"]) == 1 for cu in bcw_units) or i, i                          # ... also where the slice has explicit weights
    lm = jobs["lmcs_lut"] != 0
    assert lm.any() and not (lm & (jobs["chroma"] != 0)).any() and (~lm & (jobs["chroma"] == 0)).any(), i
    assert set(np.unique(jobs["hf_idx"])) == {0, 1} and not jobs["hf_idx"][jobs["chroma"] != 0].any(), i
    if p.chroma and p.hs:
        to_plane = (jobs["chroma"] != 0) & (jobs["w"] <= 2)
        assert to_plane.any() and np.all(jobs["dst"][to_plane] >> 40 == 1) and np.all(jobs["dst"][~to_plane] >> 40 == 5), i
        assert any(cc.plane_mask(p, c).any() for c in (1, 2)), i
    # the command array: patched, named-but-mismatched, unnamed and foreign commands all occur
    want = cc.expect_cmds(p, 5 << 40)
    ciip = p.cmds["kind"] == abi.RECON_CIIP
    changed = (want["resid"] != p.cmds["resid"]) | (want["joint"] != p.cmds["joint"])
    assert changed.any() and not changed[~ciip].any() and (ciip & ~changed).any() and (~ciip).sum() > len(p.cus), i
    assert set(want["joint"][changed].tolist()) == {1, 2, 3}, i
    assert not cc.region_mask(p).all() and cc.region_mask(p).mean() > 0.9, i
    return sizes, found


def test_the_case_list_holds_what_the_gpu_test_relies_on():
    sizes, found = set(), dict(slice_above=0, tile_left=0, tile_above=0, picture_top=0, picture_left=0)
    for i in range(len(cc.CASES)):
        s, f = _check_picture(i, cc.case_picture(i))
        sizes |= s
        for k, v in f.items():
            found[k] += v
    assert sizes >= {(4, 16), (16, 4), (8, 8), (64, 64), (32, 8), (64, 16)}, sizes
    assert all(v > 0 for v in found.values()), found
    assert {c[0] for c in cc.CASES} == {8, 10, 12} and {c[1] for c in cc.CASES} == {0, 1, 2, 3} and {c[2] for c in cc.CASES} == {5, 6, 7}


def test_weight_restatement_by_hand():
    """A 2 x 2 CTU picture with one unit per CTU corner case: the flags of ff_vvc_decode_neighbour decide whether an intra neighbour counts."""
    p = cc.CiipPicture(128, 128, 6, 1, 2)
    p.mvf["pred_flag"] = 0                                   # everything around is intra
    assert cc.intra_weight(p, 0, 0, 8, 8) == 1              # picture corner: no neighbour
    assert cc.intra_weight(p, 8, 0, 8, 8) == 2 and cc.intra_weight(p, 0, 8, 8, 8) == 2 and cc.intra_weight(p, 8, 8, 8, 8) == 3
    assert cc.intra_weight(p, 64, 64, 8, 8) == 3            # CTU corner, same slice, same tile
    p.slice_idx[:] = [0, 0, 1, 1]
    assert cc.intra_weight(p, 64, 64, 8, 8) == 2 and cc.intra_weight(p, 64, 72, 8, 8) == 3        # slice edge above; no slice test on the left
    p.slice_idx[:] = [0, 1, 2, 3]
    assert cc.intra_weight(p, 64, 0, 8, 8) == 2             # the left CTU is another slice: still available
    p.slice_idx[:] = 0
    p.col_bd[:] = [0, 1, 2]
    assert cc.intra_weight(p, 64, 64, 8, 8) == 2 and cc.intra_weight(p, 72, 64, 8, 8) == 3        # tile edge on the left
    p.col_bd[:] = [0, 0, 2]
    p.row_bd[:] = [0, 1, 2]
    assert cc.intra_weight(p, 64, 64, 8, 8) == 2 and cc.intra_weight(p, 64, 72, 8, 8) == 3        # tile edge above
    p.mvf[15, 17]["pred_flag"] = 1                           # the unit's upper neighbour entry is ((x0 + w - 1) >> 2, (y0 - 1) >> 2)
    p.row_bd[:] = [0, 0, 2]
    assert cc.intra_weight(p, 64, 64, 8, 8) == 2 and cc.intra_weight(p, 64, 64, 4, 16) == 3


def test_malformed_list_is_what_it_says():
    p = cc.case_picture(0)
    q, where = cc.with_malformed(p)
    assert sorted(where) == sorted(cc.MALFORMED) and len(q.cus) == len(p.cus) + len(cc.MALFORMED)
    ok = np.array([cc.unit_ok(q, cu) for cu in q.cus])
    assert sorted(np.nonzero(~ok)[0].tolist()) == sorted(where.values())
    assert np.all(np.diff(q.cus["first_job"].astype(np.int64)) > 0)
    # every malformed record is malformed in its own way only: repairing that one thing makes it acceptable
    last = q.cus[where["first_job past n_jobs"]]
    assert cc.unit_ok(q, last, n_jobs=q.n_jobs + 1) and int(last["first_job"]) < q.n_jobs
    r = q.cus[where["region past scratch_len"]].copy()
    assert int(r["scratch_off"]) < q.scratch_len
    r["scratch_off"] = 0
    assert cc.unit_ok(q, r)
    r = q.cus[where["slice out of range"]].copy()
    r["slice"] = 1
    assert cc.unit_ok(q, r)
    for name, pf in (("pred_flag 0", 0), ("ref_idx 16", 1)):
        cu = q.cus[where[name]]
        m = q.mvf[int(cu["y0"]) >> 2, int(cu["x0"]) >> 2]
        assert int(m["pred_flag"]) == pf and (pf == 0 or int(m["ref_idx"][0]) == 16)
    # the commands they name exist, are CIIP commands and carry the records' own geometry
    want = cc.expect_cmds(q, 5 << 40)
    for i in where.values():
        for c in range(3):
            k = q.cmds[int(q.cus[i]["cmd"][c])]
            assert k["kind"] == abi.RECON_CIIP and k["c_idx"] == c and (k["x0"], k["y0"], k["w"], k["h"]) == tuple(q.cus[i][n] for n in ("x0", "y0", "cb_width", "cb_height"))
    assert np.array_equal(want[len(p.cmds):], q.cmds[len(p.cmds):])


def test_end_to_end_picture_mixes_the_three_kinds():
    work, p = cc.e2e_work()
    assert all(cc.unit_ok(p, cu) for cu in p.cus) and len(p.cus) > 20
    pf = p.mvf["pred_flag"]
    assert (pf == 0).mean() > 0.1 and ((pf != 0) & (p.mvf["ciip_flag"] == 0)).mean() > 0.1 and (p.mvf["ciip_flag"] == 1).mean() > 0.1
    assert set(cc.unit_weights(p).tolist()) == {1, 2, 3}
    named = p.cus["cmd"].reshape(-1)
    assert np.all(named < len(p.cmds)) and np.all(p.cmds["kind"][named] == abi.RECON_CIIP) and len(set(named.tolist())) == len(named)
    assert (work.cmds["kind"] == abi.RECON_CIIP).sum() == len(named)
    want = cc.expect_cmds(p, 0)
    assert np.array_equal(want["resid"][named], work.cmds["resid"][named] * p.isz)             # the regions are recon_cases' offsets
    assert len(np.unique(p.slice_idx)) == 2 and len(np.unique(p.col_bd)) > 2

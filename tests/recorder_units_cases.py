"""The recorder's unit entry (vvc355_rec_ctu_units / vvc355_rec_units, include/vvc_mi355_rec.h) on pictures with CIIP units and motion.

A picture is a ref_recon_cases drawing (a listed one redrawn from its seed, or a sweep picture: nobody writes to that module's own
objects) changed in three ways, all seeded:
  * eligible inter units (single tree, sides 4..64, area >= 64) become CIIP units;
  * an uncoded unit gets the transform units skipped_transform_tree_unit makes for it (one per 64x64 tile, nothing coded): the walk
    ignores them, the unit records need them;
  * every inter unit gets a prediction unit `cu["pu"]`: PLAIN (one MvField, or a grid of 8x8 sub-blocks), AFFINE or GPM.

The expectations are numpy written from the rules of INTEGRATION.md section 3 and call no C:
  derive()        ref_recon_cases.derive() extended by the CIIP rules (PRED + CIIP commands, KEEP for every block of a CIIP unit, a CTU
                  with a CIIP unit counts as one with an intra unit), in the form recorder_cases.differences() compares;
  expect_units()  the cu / tu records with their QP bytes, the motion records and the inter / affine / GPM / CIIP lists per CTU, with
                  the running sums;
  paint_*()       the QP tables and the MvField table painted straight from the units, for the comparison through tables.
Used by tests/test_recorder_units_cpu.py, tests/test_recorder_units_gpu.py and tools/recorder_units_time.py."""
import ctypes
from collections import Counter
from types import SimpleNamespace

import numpy as np

import ciip_frame_cases as cf
import inter_tb_cases as tc
import intra_tb_cases as itc
import mvf_unit_cases as mu
import qp_rec_cases as qc
import recorder_cases as rk
import ref_recon_cases as rc
import ts_tb_cases as ts
from ffvvc_amd import abi

SEED = 0x2EC0C11B
PU = np.dtype(abi.RecPu, align=True)
REC, UNIT, MVF = qc.REC_DT, mu.UNIT_DT, mu.MVF_DT
INTER_PU, AFFINE_CU, GPM_CU, CIIP_CU = (np.dtype(t, align=True) for t in (abi.InterPu, abi.AffineCu, abi.GpmCu, abi.CiipCu))
NO_CMD = abi.CIIP_NO_CMD
_cmd = rc._cmd
LISTS = ("cu", "cu_qp", "tu", "tu_qp_c", "first_cu", "first_tu", "mvf", "first_mvf", "inter", "affine", "gpm", "ciip")
TOTALS = ("n_inter_jobs", "n_affine_jobs", "n_gpm_jobs", "n_ciip_jobs", "ciip_scratch_len")

# listed pictures: ref_recon_cases' own drawings (CTU 32 / 64 / 128 with partial CTUs right and below, every chroma format, LMCS on and off,
# slices, tiles) and the fraction of eligible inter units that become CIIP units
_LISTED = {"U0": ("T0", 0.5), "U1": ("T1", 0.4), "U2": ("T2", 0.4), "U3": ("T3", 0.5), "U4": ("T4", 0.5), "U5": ("T5", 0.35), "U6": ("T6", 0.5),
           "U7": ("T7", 0.5), "U8": ("T8", 0.35), "U9": ("T9", 0.5), "UD": ("directed", 1.0)}
GPU_CIIP = ("U1", "U5", "U2")                 # 8 / 10 / 12 bit
GPU_UNITS = ("V64", "V128")                   # units_picture(): CTU 64, CTU 128


def tiles16(v):
    return (v + 15) // 16


# ---------------------------------------------------------------------------------------------------------------- drawing

def _motion_field(rng, ciip=0):
    pf = int(rng.integers(1, 4))
    ref = [int(rng.integers(0, 2)) if pf & 1 else -1, int(rng.integers(0, 2)) if pf & 2 else -1]
    hpel = int(rng.random() < 0.2)
    mv = rng.integers(-48, 49, size=(2, 2))
    if hpel:
        mv = mv // 8 * 8
    bcw = int(rng.integers(1, 5)) if pf == 3 and rng.random() < 0.3 else 0
    return mu.mvfield(mv * np.array([[pf & 1], [pf >> 1]]), ref, hpel, bcw, pf, ciip)


def draw_pu(rng, pic, cu):
    """The prediction unit of an inter unit: dict(kind, msf, nsx, nsy, dmvr, bdof, hpel, bcw, pred_flag, model, part, ref_idx, motion int32)."""
    w, h = cu["w"], cu["h"]
    pu = dict(kind=mu.PLAIN, msf=0, nsx=1, nsy=1, dmvr=0, bdof=0, hpel=0, bcw=0, pred_flag=0, model=0, part=0, ref_idx=[0, 0])
    r = rng.random()
    if cu["ciip_flag"]:
        m = _motion_field(rng, int(rng.random() < 0.5))                 # the recorder sets ciip_flag in the record whatever the field says
        pu.update(hpel=int(m["hpel_if_idx"]), motion=np.frombuffer(m.tobytes(), "<i4").copy())
    elif r < 0.2 and w >= 8 and h >= 8:
        pf = int(rng.integers(1, 4))
        base = rng.integers(-40, 41, size=(2, 1, 2))
        cp = base + rng.integers(-6, 7, size=(2, 3, 2)) * (rng.random() < 0.85)
        pu.update(kind=mu.AFFINE, model=int(rng.integers(1, 3)), pred_flag=pf, hpel=0, bcw=int(rng.integers(0, 5)) if pf == 3 else 0,
                  ref_idx=[int(rng.integers(0, 2)) if pf & 1 else -1, int(rng.integers(0, 2)) if pf & 2 else -1],
                  msf=int(rng.random() < 0.5), motion=np.ascontiguousarray(cp, "<i4").reshape(12))
    elif r < 0.35 and 8 <= w <= 64 and 8 <= h <= 64 and w < 8 * h and h < 8 * w:
        parts = []
        for _ in range(2):
            l = int(rng.integers(0, 2))
            mv = np.zeros((2, 2), np.int64)
            mv[l] = rng.integers(-48, 49, size=2)
            parts.append(mu.mvfield(mv, [int(rng.integers(0, 2)) if k == l else -1 for k in range(2)], 0, 0, 1 << l))
        pu.update(kind=mu.GPM, part=int(rng.integers(0, 64)), msf=0, motion=np.frombuffer(parts[0].tobytes() + parts[1].tobytes(), "<i4").copy())
    elif r < 0.5 and w >= 8 and h >= 8:                                   # sub-block temporal merge: own motion per 8x8
        nsx, nsy = w // 8, h // 8
        fields = b"".join(_motion_field(rng).tobytes() for _ in range(nsx * nsy))
        pu.update(msf=1, nsx=nsx, nsy=nsy, motion=np.frombuffer(fields, "<i4").copy())
    else:
        m = _motion_field(rng)
        bi = int(m["pred_flag"]) == 3 and not int(m["bcw_idx"])
        big = bi and w >= 8 and h >= 8 and w * h >= 128                 # the parser's rule for DMVR / BDOF, then in 16x16 sub-blocks of one motion
        dmvr, bdof = int(big and rng.random() < 0.5), int(big and rng.random() < 0.5)
        nsx, nsy = (max(1, w // 16), max(1, h // 16)) if (dmvr or bdof) else (1, 1)
        pu.update(hpel=int(m["hpel_if_idx"]), dmvr=dmvr, bdof=bdof, nsx=nsx, nsy=nsy, motion=np.tile(np.frombuffer(m.tobytes(), "<i4"), nsx * nsy).copy())
    return pu


def ciip_eligible(cu):
    return cu["pred_mode"] == 0 and cu["tree_type"] == 0 and 4 <= cu["w"] <= 64 and 4 <= cu["h"] <= 64 and cu["w"] * cu["h"] >= 64


def dress(pic, seed, ciip_frac):
    """The three changes of the module docstring on a freshly drawn picture (in place); returns it."""
    rng = np.random.default_rng([SEED, seed])
    for ctu in pic.ctus:
        for cu in ctu:
            if ciip_eligible(cu) and rng.random() < ciip_frac:
                cu["ciip_flag"] = 1
            if not cu["coded_flag"] and not cu["tus"]:
                cu["tus"] = [dict(x0=cu["x0"] + dx, y0=cu["y0"] + dy, w=min(cu["w"], 64), h=min(cu["h"], 64), coded=[0, 0, 0], joint=0, tbs=[])
                             for dy in range(0, cu["h"], 64) for dx in range(0, cu["w"], 64)]
            if cu["pred_mode"] != 1 and cu["tree_type"] != 2:
                cu["pu"] = draw_pu(rng, pic, cu)
    pic._flat = None
    return pic


def directed_picture():
    """One CTU of 128 without an intra unit: three inter units of 64x64, the one at (64, 0) with coded Cb and Cr, and a last unit at (64, 64)
    that dress() turns into a CIIP unit: the two chroma blocks are kept by a unit recorded after them."""
    pic = rc.draw("directed", 0xD1EC, bd=10, idc=1, ctb_log2=7, size=(128, 128), intra=0.0, slices=[(0, 1)], lmcs=True, inter_ctu=1.0)
    rng = np.random.default_rng(0xD1ED)
    sl = pic.slices[0]
    units = []
    for (x, y) in ((0, 0), (64, 0), (0, 64), (64, 64)):
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
    pic.ctus, pic._flat = [units], None
    return pic


_pictures = {}


def picture_names():
    return list(_LISTED)


def picture(name):
    """A listed picture; made once, nobody writes to it."""
    if name not in _pictures:
        base, frac = _LISTED[name]
        if base == "directed":
            pic = dress(directed_picture(), 99, 0.0)
            pic.ctus[0][3]["ciip_flag"] = 1
            pic.ctus[0][3]["pu"] = draw_pu(np.random.default_rng(SEED), pic, pic.ctus[0][3])
        else:
            k = list(rc._LISTED).index(base)
            pic = dress(rc.draw(name, rc.SEED + k, **rc._LISTED[base]), k, frac)
        pic.name = name
        _pictures[name] = pic
    return _pictures[name]


def units_picture(name):
    """The pictures whose unit lists go through the deblocking passes: T8's and T2's drawings without ISP (its parts 1 and 2 samples wide
    have records that paint nothing, by the passes' rule for rectangles that are no multiples of 4), CIIP units and motion as everywhere."""
    base = dict(V64="T8", V128="T2")[name]
    k = list(rc._LISTED).index(base)
    kw = dict(rc._LISTED[base])
    kw["tools"] = dict(kw.get("tools", {}), isp=0.0)
    pic = dress(rc.draw(name, rc.SEED + 100 + k, **kw), 100 + k, 0.35)
    assert not any(cu["isp_type"] for ctu in pic.ctus for cu in ctu)
    return pic


def sweep_picture(k):
    pic = rc.sweep_picture(k, salt=7)
    return dress(pic, 1000 + k, float(np.random.default_rng([SEED, 7, k]).choice([0.0, 0.3, 0.6])))


# ---------------------------------------------------------------------------------------------------------------- the PODs and the calls

def pods(pic):
    """recorder_cases.pods plus the vvc355_rec_pu array (one per coding unit, paired by index) and the int32 store its pointers go into."""
    p = rk.pods(pic)
    units = [cu for ctu in pic.ctus for cu in ctu]
    motion = [cu["pu"]["motion"] for cu in units if "pu" in cu]
    p.motion = np.concatenate(motion).astype(np.int32) if motion else np.zeros(1, np.int32)
    p.pus = np.zeros(max(len(units), 1), PU)
    p.motion_off = np.full(max(len(units), 1), -1, np.int64)
    at = 0
    for i, cu in enumerate(units):
        if "pu" not in cu:
            continue
        u, r = cu["pu"], p.pus[i]
        r["motion"], p.motion_off[i] = p.motion.ctypes.data + 4 * at, at
        at += len(u["motion"])
        r["kind"], r["merge_subblock_flag"], r["num_sb_x"], r["num_sb_y"], r["dmvr_flag"], r["bdof_flag"] = u["kind"], u["msf"], u["nsx"], u["nsy"], u["dmvr"], u["bdof"]
        r["hpel_if_idx"], r["bcw_idx"], r["pred_flag"], r["motion_model_idc"], r["gpm_partition_idx"], r["ref_idx"] = \
            u["hpel"], u["bcw"], u["pred_flag"], u["model"], u["part"], u["ref_idx"]
    p.has_inter = [any("pu" in cu for cu in ctu) for ctu in pic.ctus]
    return p


def feed(lib, rec, pic, p, order=None, null_pus=True):
    """vvc355_rec_ctu_units for the CTUs in `order` (raster by default), pus null for a CTU without an inter unit: the first refusal, or 0."""
    for rs in (range(len(pic.ctus)) if order is None else order):
        rs = int(rs)
        first, n = int(p.first[rs]), int(p.first[rs + 1] - p.first[rs])
        pus = None if (null_pus and not p.has_inter[rs]) else p.pus.ctypes.data + PU.itemsize * first
        ret = lib.vvc355_rec_ctu_units(rec, rs, rk.slice_flags(pic, rs), int(pic.slice_idx[rs]), p.cus.ctypes.data + rk.CU.itemsize * first, pus, n)
        if ret:
            return ret
    return 0


def units_snapshot(lib, rec, n_ctus):
    """Everything a vvc355_rec_units_result names, copied out."""
    u = abi.RecUnitsResult()
    ret = lib.vvc355_rec_units(rec, ctypes.byref(u))
    assert ret == 0, f"vvc355_rec_units: {ret}"
    s = SimpleNamespace(res=u)
    s.cu, s.cu_qp, s.tu = rk._copy(u.cu, u.n_cu, REC), rk._copy(u.cu_qp, u.n_cu, np.int8), rk._copy(u.tu, u.n_tu, REC)
    s.tu_qp_c = rk._copy(u.tu_qp_c, 2 * u.n_tu, np.int8).reshape(-1, 2)
    s.first_cu, s.first_tu, s.first_mvf = (rk._copy(q, n_ctus + 1, np.int32) for q in (u.ctu_first_cu, u.ctu_first_tu, u.ctu_first_mvf))
    s.mvf = rk._copy(u.mvf, u.n_mvf, UNIT)
    s.inter, s.affine = rk._copy(u.inter, u.n_inter, INTER_PU), rk._copy(u.affine, u.n_affine, AFFINE_CU)
    s.gpm, s.ciip = rk._copy(u.gpm, u.n_gpm, GPM_CU), rk._copy(u.ciip, u.n_ciip, CIIP_CU)
    s.totals = {k: int(getattr(u, k)) for k in TOTALS}
    d = abi.RecDeblockTus()
    ret = lib.vvc355_rec_deblock_units(rec, ctypes.byref(d))
    assert ret == 0, f"vvc355_rec_deblock_units: {ret}"
    s.tud, s.tud_qp_c, s.first_tud = rk._copy(d.tu, d.n_tu, REC), rk._copy(d.tu_qp_c, 2 * d.n_tu, np.int8).reshape(-1, 2), rk._copy(d.ctu_first_tu, n_ctus + 1, np.int32)
    return s


def record(lib, pic, pack=True, order=None, rec=None, p=None):
    """One picture through vvc355_rec_ctu_units: recorder_cases' snapshot with the unit lists as `.u`."""
    own = rec is None
    rec = lib.vvc355_rec_create() if own else rec
    try:
        p = pods(pic) if p is None else p
        par = rk.params(pic, pack)
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        ret = feed(lib, rec, pic, p, order)
        assert ret == 0, f"{pic.name}: vvc355_rec_ctu_units refused a CTU: {ret}"
        res = abi.RecResult()
        assert lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
        o = rk.snapshot(lib, rec, res)
        o.u = units_snapshot(lib, rec, len(pic.ctus))
        return o
    finally:
        if own:
            lib.vvc355_rec_destroy(rec)


# ---------------------------------------------------------------------------------------------------------------- commands and TB records

def derive(pic):
    """ref_recon_cases.derive() with CIIP units: their PRED + CIIP commands ahead of the commands of an inter unit, every coded block of
    theirs kept in the walk, and their CTU counted among those that hold an intra unit.  Returns that function's namespace; d.ciip_cmds =
    per CIIP unit in command order the indices of its CIIP commands."""
    hs, vs, ctb_log2, ncx = pic.hs, pic.vs, pic.ctb_log2, pic.ncx
    tabs = rc._tables(pic)
    has_intra = [any(cu["pred_mode"] == 1 or cu["ciip_flag"] for cu in ctu) for ctu in pic.ctus]
    sy = pic.size_y

    def ctu_of(x, y):
        return (y >> ctb_log2) * ncx + (x >> ctb_log2)

    def needs_walk(cu):
        xv, yv = cu["x0"] & ~(sy - 1), cu["y0"] & ~(sy - 1)
        return (xv > 0 and has_intra[ctu_of(xv - 1, yv)]) or (yv > 0 and has_intra[ctu_of(xv, yv - 1)])

    intra, inter, skip = [], [], []
    rid = 0
    cmds, ctus = [], np.zeros(len(pic.ctus), rc.CTU)
    kind = np.zeros(len(pic.ctus), np.int8)
    routed, walked = set(), set()
    stats = dict(keep=0, batched_scaled=0, walk_scaled=0)
    ciip_cmds = []
    for rs, ctu in enumerate(pic.ctus):
        sl = pic.slices[int(pic.slice_idx[rs])]
        out, any_resid, ciip_here = [], False, []
        for cu in ctu:
            cur = (cu["x0"], cu["y0"], cu["w"], cu["h"])
            if cu["ciip_flag"]:
                named = [NO_CMD] * 3
                for c in range(3 if pic.idc else 1):
                    if c and (cu["w"] >> hs) <= 2:
                        continue
                    out.append(_cmd(abi.RECON_PRED, c, *cur, *cur, mode=0))
                    named[c] = len(out)                                    # relative to the CTU's list; made absolute below
                    out.append(_cmd(abi.RECON_CIIP, c, *cur, *cur))
                ciip_here.append(named)
            if not cu["coded_flag"]:
                out.append(_cmd(abi.RECON_MARK, 0, *cur, *cur))
                out.append(_cmd(abi.RECON_MARK, 1, *cur, *cur))
                continue
            is_intra = cu["pred_mode"] == 1
            for ch in range(int(cu["tree_type"] == 2), 1 + int(pic.idc != 0 and cu["tree_type"] != 1)):
                for i, tu in enumerate(cu["tus"]):
                    tr = (tu["x0"], tu["y0"], tu["w"], tu["h"])
                    if not is_intra:
                        out.append(_cmd(abi.RECON_MARK, ch, *tr, *cur))
                    elif ch == 0:
                        x0, y0, w, h = tr
                        has = True
                        if cu["isp_type"] == 2 and w < 4:
                            has, w = i % (4 // w) == 0, 4
                        if has:
                            out.append(_cmd(abi.RECON_PRED, 0, x0, y0, w, h, *cur, mode=0 if cu["mip_flag"] else cu["mode_y"], ref_idx=cu["ref_idx"],
                                            is_mip=cu["mip_flag"], mip_mode=cu["mip_mode"], mip_transposed=cu["mip_transposed"],
                                            isp_split=int(cu["isp_type"] != 0), bdpcm_flag=cu["bdpcm"][0]))
                            out.append(_cmd(abi.RECON_MARK, 0, x0, y0, w, h, *cur))
                    elif cu["isp_type"] == 0 or i == len(cu["tus"]) - 1:
                        r = tr if cu["isp_type"] == 0 else cur
                        if 81 <= cu["mode_c"] <= 83:
                            out.append(_cmd(abi.RECON_CCLM, 1, *r, *cur, mode=cu["mode_c"]))
                        else:
                            direct = int(cu["mip_chroma_direct"] and cu["mip_flag"])
                            for c in (1, 2):
                                out.append(_cmd(abi.RECON_PRED, c, *r, *cur, mode=cu["mode_c"], is_mip=direct, mip_mode=cu["mip_mode"] if direct else 0,
                                                mip_transposed=cu["mip_transposed"] if direct else 0, isp_split=int(cu["isp_type"] != 0),
                                                bdpcm_flag=cu["bdpcm"][c]))
                        out.append(_cmd(abi.RECON_MARK, 1, *r, *cur))
                    for b in tu["tbs"]:
                        c = b["c_idx"]
                        if (c > 0) != ch or not b["has"]:
                            continue
                        w, h = b["w"], b["h"]
                        lw, lh = w.bit_length() - 1, h.bit_length() - 1
                        scale = 8 if (c and sl[1] and pic.chroma_scale_flag and w * h > 4) else 0
                        jb = (1 | pic.joint_sign << 1 | (tu["coded"][1] ^ tu["coded"][2]) << 2) if (tu["joint"] and c) else 0
                        qp = rc.tb_qp(pic, cu, tu, c, b["ts"])
                        x_c, y_c = b["x0"] >> (hs if c else 0), b["y0"] >> (vs if c else 0)
                        by_rule = bool(not is_intra and not cu["ciip_flag"] and scale and needs_walk(cu))
                        walk = bool(is_intra or cu["ciip_flag"] or by_rule)
                        unit_cu = (cu["x0"], cu["y0"])
                        if b["ts"]:
                            s = ts.spec(c, x_c, y_c, lw, lh, b["levels"], b["nzw"], b["nzh"], qp=qp, bdpcm=bool(cu["bdpcm"][c]),
                                        vert=bool(cu["bdpcm"][c]) and (cu["mode_c"] if c else cu["mode_y"]) == 50, joint=0 if walk else scale | jb,
                                        keep=walk, cu=unit_cu)
                            skip.append(s)
                        elif is_intra:
                            lf = bool(cu["apply_lfnst"][c])
                            flags = ((abi.TU_MTS_ENABLED if pic.mts_enabled else 0) | (abi.TU_EXPLICIT_MTS_INTRA if pic.explicit_mts_intra else 0) |
                                     (abi.TU_ISP if cu["isp_type"] else 0) | abi.TU_INTRA | (abi.TU_MIP if cu["mip_flag"] else 0))
                            s = itc.spec(lw, lh, b["levels"], 4 if lf else b["nzw"], 4 if lf else b["nzh"], c, qp, sl[0], lf, cu["lfnst_idx"],
                                         rc.lfnst_mode(pic, tabs, cu, b) if lf else 0, flags, cu["mts_idx"])
                            intra.append(s)
                        else:
                            flags = ((abi.TU_MTS_ENABLED if pic.mts_enabled else 0) | (abi.TU_SBT if cu["sbt_flag"] else 0) |
                                     (abi.TU_SBT_HORIZONTAL if cu["sbt_horizontal"] else 0) | (abi.TU_SBT_POS if cu["sbt_pos"] else 0))
                            s = tc.spec(c, x_c, y_c, lw, lh, b["levels"], b["nzw"], b["nzh"], qp=qp, dep=sl[0], tu_flags=flags, mts_idx=cu["mts_idx"],
                                        joint=0 if walk else scale | jb, keep=walk, cu=unit_cu)
                            inter.append(s)
                        s["rid"], s["ciip"], s["by_rule"], s["rs"] = rid, bool(cu["ciip_flag"]), by_rule, rs
                        rid += 1
                        unit = (cu["x0"] // sy, cu["y0"] // sy)
                        if not walk:
                            if scale:
                                routed.add(unit)
                                stats["batched_scaled"] += 1
                            continue
                        stats["keep"] += 1
                        if scale:
                            walked.add(unit)
                            stats["walk_scaled"] += by_rule                # the blocks the neighbour rule keeps; a CIIP unit's own are kept anyway
                        any_resid = True
                        out.append(_cmd(abi.RECON_RESID, c, b["x0"], b["y0"], w, h, *cur, resid=s["rid"], joint=scale))
                        if jb:
                            out.append(_cmd(abi.RECON_RESID, 3 - c, b["x0"], b["y0"], w, h, *cur, resid=s["rid"], joint=scale | jb))
        if has_intra[rs] or any_resid:
            ctus[rs]["first_cmd"], ctus[rs]["n_cmd"] = len(cmds), len(out)
            ciip_cmds += [[v if v == NO_CMD else v + len(cmds) for v in named] for named in ciip_here]
            cmds += out
            kind[rs] = 2 if has_intra[rs] else 1
    for rs in np.nonzero(kind == 1)[0]:
        rx, ry = rs % ncx, rs // ncx
        ctus[rs]["flags"] = (abi.RECON_CTU_LIGHT | (abi.RECON_CTU_LUMA_LEFT if rx and kind[rs - 1] == 2 else 0) |
                             (abi.RECON_CTU_LUMA_UP if ry and kind[rs - ncx] == 2 else 0))
    d = SimpleNamespace(pic=pic, ctus=ctus, kind=kind, routed=sorted(routed), walked=sorted(walked), stats=stats, ciip_cmds=ciip_cmds)
    d.cmds = np.array(cmds, rc.CMD) if cmds else np.zeros(0, rc.CMD)
    d.order = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
    d.intra, d.class_first = itc.group_by_class(intra)
    d.inter, d.bin_first = tc.group(inter)
    d.skip, d.ts_first = ts.group(skip)
    d.specs = d.intra + d.inter + d.skip
    d.offs, d.arena_len = tc.arena_offsets(d.specs)
    d.off_of = {s["rid"]: o for s, o in zip(d.specs, d.offs)}
    d.tpic = tc.Picture(pic.planes, pic.bd, hs, vs, sy, ctb_log2, pic.model if pic.chroma_scale_flag else None)
    return d


# ---------------------------------------------------------------------------------------------------------------- the unit lists

def _qp8(v):
    return int(np.int8(v))


def tu_records(pic, cu, tree):
    """The DEBLOCKING transform-unit records (vvc355_rec_deblock_units) of one coding unit and tree, [(x0, y0, w, h, flags, (qp_cb, qp_cr))], by the call sites of set_tb_pos /
    set_tb_tab (vvc_ctu.c:379-401, :1241-1250): one record per transform unit, bit 4 where the unit is BDPCM-coded in that tree (pcmf), but
      * the chroma blocks of an ISP unit belong to its last partition and cover the WHOLE unit: one tree-1 record over the coding unit;
      * ISP partitions 1 or 2 samples wide (high) share a 4-sample column (row) of the tables: one tree-0 record per column (row), coded
        where any of its partitions is (every partition that carried a residual wrote the flag)."""
    pcm = int(bool(cu["bdpcm"][1 if tree else 0])) << 4
    if tree:
        tus = cu["tus"][-1:] if cu["isp_type"] else cu["tus"]
        out = []
        for tu in tus:
            both = tu["joint"] and tu["coded"][1] and tu["coded"][2]
            rect = (cu["x0"], cu["y0"], cu["w"], cu["h"]) if cu["isp_type"] else (tu["x0"], tu["y0"], tu["w"], tu["h"])
            out.append(rect + (0x80 | tu["coded"][1] << 1 | tu["coded"][2] << 2 | tu["joint"] << 3 | pcm,
                               (_qp8(cu["qp"][3 if both else 1]), _qp8(cu["qp"][3 if both else 2]))))
        return out
    tus = cu["tus"]
    if cu["isp_type"] and (tus[0]["w"] < 4 or tus[0]["h"] < 4):
        ver = tus[0]["w"] < 4
        per = 4 // (tus[0]["w"] if ver else tus[0]["h"])
        out = []
        for g in range(0, len(tus), per):
            coded = int(any(tu["coded"][0] for tu in tus[g:g + per]))
            rect = (tus[g]["x0"], tus[g]["y0"], 4, tus[g]["h"]) if ver else (tus[g]["x0"], tus[g]["y0"], tus[g]["w"], 4)
            out.append(rect + (coded | pcm, (0, 0)))
        return out
    return [(tu["x0"], tu["y0"], tu["w"], tu["h"], tu["coded"][0] | pcm, (0, 0)) for tu in tus]


def expect_units(pic, d):
    """The unit lists by the rules of INTEGRATION.md section 3, CTUs in raster order, decoding order inside a CTU: a namespace with the
    fields of units_snapshot()."""
    chroma = pic.idc != 0
    cu_l, cu_qp, tu_l, tu_qp, mv_l, first = [], [], [], [], [], {k: [0] for k in ("cu", "tu", "mvf", "tud")}
    tud_l, tud_qp = [], []
    inter, affine, gpm, ciip = [], [], [], []
    jobs = dict.fromkeys(TOTALS, 0)
    for rs, ctu in enumerate(pic.ctus):
        sl = int(pic.slice_idx[rs])
        for cu in ctu:
            x, y, w, h = cu["x0"], cu["y0"], cu["w"], cu["h"]
            pu = cu.get("pu")
            if cu["tree_type"] != 2:
                cu_l.append((x, y, w, h, (pu["msf"] | (pu["kind"] == mu.AFFINE) << 1) if pu else 0, 0))
                cu_qp.append(_qp8(cu["qp"][0]))
            for tree in range(int(cu["tree_type"] == 2), 1 + int(chroma and cu["tree_type"] != 1)):
                for tu in cu["tus"]:
                    both = tu["joint"] and tu["coded"][1] and tu["coded"][2]
                    flags = (0x80 | tu["coded"][1] << 1 | tu["coded"][2] << 2 | tu["joint"] << 3) if tree else tu["coded"][0]
                    tu_l.append((tu["x0"], tu["y0"], tu["w"], tu["h"], flags, 0))
                    tu_qp.append((_qp8(cu["qp"][3 if both else 1]), _qp8(cu["qp"][3 if both else 2])) if tree else (0, 0))
                for (tx, ty, tw, th, flags, qp_c) in tu_records(pic, cu, tree):
                    tud_l.append((tx, ty, tw, th, flags, 0))
                    tud_qp.append(qp_c)
            if cu["tree_type"] == 2:
                continue
            if pu is None:
                mv_l.append(mu.plain(x, y, w, h, mu.mvfield()))
            elif pu["kind"] == mu.PLAIN:
                sw, sh = w // pu["nsx"], h // pu["nsy"]
                for k in range(pu["nsx"] * pu["nsy"]):
                    m = pu["motion"][6 * k:6 * k + 6].copy().view(MVF)[0].copy()
                    m["ciip_flag"] |= cu["ciip_flag"]
                    mv_l.append(mu.plain(x + (k % pu["nsx"]) * sw, y + (k // pu["nsx"]) * sh, sw, sh, m))
                if cu["ciip_flag"]:
                    wc, hc = w >> pic.hs, h >> pic.vs
                    ciip.append((x, y, w, h, pu["hpel"], sl, (0, 0), jobs["n_ciip_jobs"], jobs["ciip_scratch_len"], tuple(d.ciip_cmds[len(ciip)])))
                    jobs["n_ciip_jobs"] += tiles16(w) * tiles16(h) + (2 * tiles16(wc) * tiles16(hc) if chroma else 0)
                    jobs["ciip_scratch_len"] += w * h + (2 * wc * hc if chroma and wc > 2 else 0)
                else:
                    inter.append((x, y, w, h, pu["nsx"], pu["nsy"], pu["dmvr"], pu["bdof"], 0, pu["hpel"], sl, 0, jobs["n_inter_jobs"]))
                    jobs["n_inter_jobs"] += pu["nsx"] * pu["nsy"] * tiles16(sw) * tiles16(sh)
            elif pu["kind"] == mu.AFFINE:
                mv_l.append(mu.affine(x, y, w, h, pu["model"], pu["pred_flag"], pu["motion"].reshape(2, 3, 2), pu["ref_idx"], pu["hpel"], pu["bcw"], len(affine)))
                affine.append((x, y, w, h, w >> 2, h >> 2, 0, sl, jobs["n_affine_jobs"], np.zeros((2, 2, 16), np.int16)))
                jobs["n_affine_jobs"] += (w >> 2) * (h >> 2)
            else:
                parts = pu["motion"].view(MVF)
                mv_l.append(mu.gpm(x, y, w, h, pu["part"], parts[0], parts[1]))
                gpm.append((x, y, w, h, pu["part"], sl, (0, 0), jobs["n_gpm_jobs"], pu["motion"].tobytes()))
                jobs["n_gpm_jobs"] += tiles16(w) * tiles16(h) + (2 * tiles16(w >> pic.hs) * tiles16(h >> pic.vs) if chroma else 0)
        first["cu"].append(len(cu_l)), first["tu"].append(len(tu_l)), first["mvf"].append(len(mv_l)), first["tud"].append(len(tud_l))
    e = SimpleNamespace(totals=jobs)
    e.cu, e.tu = np.array(cu_l, REC) if cu_l else np.zeros(0, REC), np.array(tu_l, REC) if tu_l else np.zeros(0, REC)
    e.cu_qp, e.tu_qp_c = np.array(cu_qp, np.int8), np.array(tu_qp, np.int8).reshape(-1, 2)
    e.first_cu, e.first_tu, e.first_mvf = (np.array(first[k], np.int32) for k in ("cu", "tu", "mvf"))
    e.tud, e.tud_qp_c = np.array(tud_l, REC) if tud_l else np.zeros(0, REC), np.array(tud_qp, np.int8).reshape(-1, 2)      # vvc355_rec_deblock_units
    e.first_tud = np.array(first["tud"], np.int32)
    e.mvf = np.array(mv_l, UNIT) if mv_l else np.zeros(0, UNIT)
    e.inter = np.array(inter, INTER_PU) if inter else np.zeros(0, INTER_PU)
    e.affine = np.array(affine, AFFINE_CU) if affine else np.zeros(0, AFFINE_CU)
    e.ciip = np.array(ciip, CIIP_CU) if ciip else np.zeros(0, CIIP_CU)
    e.gpm = np.zeros(len(gpm), GPM_CU)
    for i, g in enumerate(gpm):
        raw = np.zeros(1, GPM_CU)
        for k, v in zip(("x0", "y0", "cb_width", "cb_height", "partition_idx", "slice", "pad_", "first_job"), g[:8]):
            raw[k] = v
        raw.view(np.uint8)[GPM_CU.fields["gpm_mv"][1]:] = np.frombuffer(g[8], np.uint8)
        e.gpm[i] = raw[0]
    return e


def geometry(pic):
    return qc.geometry(pic.width, pic.height, pic.ctb_log2)


def _per_ctu_sets(first, *arrays):
    """Per CTU the multiset of the records' bytes (the arrays are paired by index)."""
    rows = [np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1) for a in arrays]
    joined = np.concatenate(rows, axis=1) if len(rows[0]) else np.zeros((0, 1), np.uint8)
    return [Counter(bytes(r) for r in joined[first[rs]:first[rs + 1]]) for rs in range(len(first) - 1)]


def paint_qp(pic):
    """The QP tables painted straight from the units (set_qp_y over the coding unit, set_qp_c_tab over the chroma transform unit): rectangles
    that are no multiples of 4 (ISP parts 1 or 2 wide) paint nothing, as their records paint nothing."""
    g = geometry(pic)
    out = {k: np.zeros((g.th, g.tw), np.int8) for k in qc.TABLES}
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] != 2:
                out["qp_y"][cu["y0"] // 4:(cu["y0"] + cu["h"]) // 4, cu["x0"] // 4:(cu["x0"] + cu["w"]) // 4] = _qp8(cu["qp"][0])
            if pic.idc and cu["tree_type"] != 1:
                for tu in cu["tus"]:
                    if (tu["x0"] | tu["y0"] | tu["w"] | tu["h"]) & 3:
                        continue
                    both = tu["joint"] and tu["coded"][1] and tu["coded"][2]
                    s = np.s_[tu["y0"] // 4:(tu["y0"] + tu["h"]) // 4, tu["x0"] // 4:(tu["x0"] + tu["w"]) // 4]
                    out["qp_c0"][s], out["qp_c1"][s] = _qp8(cu["qp"][3 if both else 1]), _qp8(cu["qp"][3 if both else 2])
    return out


def paint_mvf(pic, table, cus=None):
    """The MvField table (and prof_flags / diff_mv of the affine records, in unit order) painted straight from the units with the numpy of
    mvf_unit_cases; entries no luma-tree unit covers keep their bytes."""
    n_aff = 0
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] == 2:
                continue
            x, y, w, h, pu = cu["x0"], cu["y0"], cu["w"], cu["h"], cu.get("pu")
            if pu is None:
                e = np.zeros((h // 4, w // 4), MVF)
            elif pu["kind"] == mu.PLAIN:
                e = np.repeat(np.repeat(pu["motion"].view(MVF).reshape(pu["nsy"], pu["nsx"]), h // pu["nsy"] // 4, axis=0), w // pu["nsx"] // 4, axis=1).copy()
                e["ciip_flag"] |= cu["ciip_flag"]
            elif pu["kind"] == mu.AFFINE:
                r = mu.affine(x, y, w, h, pu["model"], pu["pred_flag"], pu["motion"].reshape(2, 3, 2), pu["ref_idx"], pu["hpel"], pu["bcw"])
                e, flags, dmv, _ = mu.affine_unit(r)
                if cus is not None:
                    cus[n_aff]["prof_flags"], cus[n_aff]["diff_mv"] = flags, dmv
                n_aff += 1
            else:
                parts = pu["motion"].view(MVF)
                e = mu.gpm_unit(mu.gpm(x, y, w, h, pu["part"], parts[0], parts[1]))[0]
            table[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = e
    return table


def unit_differences(pic, d, o):
    """What of the recorder's unit lists differs from the expectation, by name; [] = equal."""
    u, e, bad = o.u, expect_units(pic, d), []
    g = geometry(pic)

    def cmp(name, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
            bad.append(name)

    for k in ("first_cu", "first_tu", "first_mvf", "first_tud", "inter", "affine", "gpm", "ciip"):        # byte for byte
        cmp(k, getattr(u, k), getattr(e, k))
    if u.totals != e.totals:
        bad.append(f"totals {u.totals} against {e.totals}")
    if bad:
        return bad
    # cu / tu records with their sidecars and the motion records: as sets per CTU ...
    tree1 = ((u.tu["flags"] & 0x80) != 0)[:, None]
    if _per_ctu_sets(u.first_cu, u.cu, u.cu_qp) != _per_ctu_sets(e.first_cu, e.cu, e.cu_qp):
        bad.append("cu records / cu_qp")
    if _per_ctu_sets(u.first_tu, u.tu, np.where(tree1, u.tu_qp_c, 0)) != _per_ctu_sets(e.first_tu, e.tu, e.tu_qp_c):
        bad.append("tu records / tu_qp_c")
    tree1 = ((u.tud["flags"] & 0x80) != 0)[:, None]
    if _per_ctu_sets(u.first_tud, u.tud, np.where(tree1, u.tud_qp_c, 0)) != _per_ctu_sets(e.first_tud, e.tud, e.tud_qp_c):
        bad.append("deblocking tu records / their tu_qp_c")
    if _per_ctu_sets(u.first_mvf, u.mvf) != _per_ctu_sets(e.first_mvf, e.mvf):
        bad.append("mvf_unit records")
    # ... and through the tables they paint
    got = qc.expected(qc.Pic(g=g, cu=u.cu, tu=u.tu, cu_first=u.first_cu, tu_first=u.first_tu, cu_qp=u.cu_qp, tu_qp_c=u.tu_qp_c))
    want = paint_qp(pic)
    bad += [f"painted {k}" for k in qc.TABLES if not np.array_equal(got[k], want[k]) and (pic.idc or k == "qp_y")]
    mg = mu.Geo(pic.width, pic.height, pic.ctb_log2)
    if pic.width % 4 == 0 and pic.height % 4 == 0:
        t_got, t_want = mu.sentinel_table(mg), mu.sentinel_table(mg)
        c_got, c_want = mu.sentinel_cus(len(u.affine)), mu.sentinel_cus(len(u.affine))
        ok = mu.expect_table(mg, u.mvf, u.first_mvf, t_got, len(u.affine))
        mu.expect_affine_cus(mg, u.mvf, u.first_mvf, c_got)
        if not ok.all():
            bad.append("a motion record the pass would not place")
        paint_mvf(pic, t_want, c_want)
        if t_got.tobytes() != t_want.tobytes():
            bad.append("painted MvField table")
        if c_got.tobytes() != c_want.tobytes():
            bad.append("prof_flags / diff_mv by link")
    return bad


# ---------------------------------------------------------------------------------------------------------------- what the pictures reach

def census(pic, d):
    n = Counter()
    ctb = 1 << pic.ctb_log2
    n[f"ctu {ctb}"] += 1
    n[f"ctu {ctb} partial right and below"] += bool(pic.width % ctb and pic.height % ctb)
    n[f"format {pic.idc}"] += 1
    n["lmcs on" if pic.chroma_scale_flag or any(s[1] for s in pic.slices) else "lmcs off"] += 1
    n["two slices"] += len(pic.slices) >= 2
    n["tiles"] += len(set(pic.col_bd[:-1].tolist())) > 1
    only_ciip = [any(cu["ciip_flag"] for cu in ctu) and not any(cu["pred_mode"] == 1 for cu in ctu) for ctu in pic.ctus]
    for rs, ctu in enumerate(pic.ctus):
        n["ctu without an inter unit: null pus"] += bool(ctu) and not any("pu" in cu for cu in ctu)
        for cu in ctu:
            pu = cu.get("pu")
            if pu is not None:
                pfs = [pu["pred_flag"]] if pu["kind"] == mu.AFFINE else [int(m["pred_flag"]) for m in pu["motion"].view(MVF)]
                if pu["kind"] == mu.GPM:
                    pfs = [pfs[0] | pfs[1]] + pfs
                for pf in pfs:
                    n[f"kind {pu['kind']} pred_flag {pf}"] += 1
                n["sub-block plain unit"] += pu["kind"] == mu.PLAIN and pu["nsx"] * pu["nsy"] > 1
                n[f"affine model {pu['model']}"] += pu["kind"] == mu.AFFINE
            if not cu["ciip_flag"]:
                continue
            tbs = [(tu, b) for tu in cu["tus"] for b in tu["tbs"] if b["has"]] if cu["coded_flag"] else []
            n["uncoded ciip unit"] += not cu["coded_flag"]
            n["ciip unit with a luma residual"] += any(b["c_idx"] == 0 for _, b in tbs)
            n["ciip unit with a transform-skip block"] += any(b["ts"] for _, b in tbs)
            n["ciip unit with a joint cb-cr unit"] += any(tu["joint"] and b["c_idx"] for tu, b in tbs)
            n["4-wide ciip unit at 4:2:0, coded unblended chroma"] += pic.idc == 1 and cu["w"] == 4 and any(b["c_idx"] for _, b in tbs)
            n["8-wide ciip unit at 4:2:2, blended chroma"] += pic.idc == 2 and cu["w"] == 8
    sy = pic.size_y
    for s in d.specs:
        if s.get("by_rule"):
            # the CTUs whose luma decides: left of / above the unit's 64x64 unit
            xv, yv = s["cu"][0] & ~(sy - 1), s["cu"][1] & ~(sy - 1)
            deps = [(yy >> pic.ctb_log2) * pic.ncx + (xx >> pic.ctb_log2) for xx, yy, ok in ((xv - 1, yv, xv > 0), (xv, yv - 1, yv > 0)) if ok]
            walks = [r for r in deps if d.kind[r] == 2]
            n["scaled block kept because of a ctu whose only walk-written luma is a ciip unit's"] += bool(walks) and all(only_ciip[r] for r in walks)
    return n


PREMISES = (["ctu 32 partial right and below", "ctu 64 partial right and below", "ctu 128 partial right and below", "format 0", "format 1", "format 2",
             "format 3", "lmcs on", "lmcs off", "two slices", "tiles", "ctu without an inter unit: null pus", "sub-block plain unit", "affine model 1",
             "affine model 2", "uncoded ciip unit", "ciip unit with a luma residual", "ciip unit with a transform-skip block",
             "ciip unit with a joint cb-cr unit", "4-wide ciip unit at 4:2:0, coded unblended chroma", "8-wide ciip unit at 4:2:2, blended chroma",
             "scaled block kept because of a ctu whose only walk-written luma is a ciip unit's"] +
            [f"kind {k} pred_flag {pf}" for k in (mu.PLAIN, mu.AFFINE, mu.GPM) for pf in (1, 2, 3)])


# ---------------------------------------------------------------------------------------------------------------- the stand-alone check

def digest(o):
    """What tools/recorder_units_check.c prints for a run: recorder_cases.digest()'s bytes, then the unit lists and their totals."""
    u = o.u
    return rk.fnv1a(o.head, o.cmds.view(np.uint8), o.ctus.view(np.uint8), o.intra.view(np.uint8), o.inter.view(np.uint8), o.ts.view(np.uint8),
                    o.lv.view(np.uint8), o.levels.view(np.uint8), o.arena.view(np.uint8),
                    u.cu.view(np.uint8), u.cu_qp.view(np.uint8), u.tu.view(np.uint8), np.ascontiguousarray(u.tu_qp_c).view(np.uint8),
                    u.first_cu.view(np.uint8), u.first_tu.view(np.uint8), u.mvf.view(np.uint8), u.first_mvf.view(np.uint8), u.inter.view(np.uint8),
                    u.affine.view(np.uint8), u.gpm.view(np.uint8), u.ciip.view(np.uint8), np.array([u.totals[k] for k in TOTALS], np.int32).view(np.uint8))


def dump(pic, path, pack=True):
    """recorder_cases.dump()'s file, then: int32 count of motion elements, the slice index per CTU (int32), the vvc355_rec_pu array with an
    element index in place of the pointer (NO_LEVELS = none), the int32 motion store."""
    rk.dump(pic, path, pack)
    p = pods(pic)
    n_cu = p.n_cu
    pus = p.pus[:n_cu].copy()
    pus["motion"] = np.where(p.motion_off[:n_cu] >= 0, p.motion_off[:n_cu], -1).astype(np.int64).view(np.uint64) if n_cu else 0
    with open(path, "ab") as f:
        f.write(np.array([len(p.motion)], np.int32).tobytes())
        f.write(pic.slice_idx.astype(np.int32).tobytes())
        f.write(pus.tobytes())
        f.write(p.motion.astype(np.int32).tobytes())

"""Whole DECODED pictures — the pictures of ref_picture_cases carried on through deblocking, SAO and ALF — pinned against the reference's own
filter callers run on the reference's own reconstruction (ref_decode_picture, then ref_deblock_picture, ref_sao_picture, ref_alf_picture of
oracle/ref_shim_filter.c, composed from Python: no new shim entry).

ONE unit description per picture (a ref_picture_cases picture: W0-W9, the quiet pictures Q0-Q2 below, the sweep's draws) and both sides
derived from it:

  reference side   reference_tables(): the side tables the reference's deblocking reads (bs_cases.BsTables.IN), painted in numpy STRAIGHT
                   FROM THE UNITS by the rules of vvc_ctu.c — set_cb_pos / set_cb_tab over a coding unit, set_tb_pos / set_tb_tab over a
                   transform BLOCK (a coded flag only where the block carried a residual, the joint flag over the Cb block, the pcm flag
                   where the unit is BDPCM-coded), set_qp_y over every unit (uncoded ones too), set_qp_c_tab (the joint entry of cu->qp[]
                   where the TU is joint and both chroma blocks are coded).  mvf is the UNREFINED table (recorder_units_cases.paint_mvf,
                   ciip_flag set for CIIP units).  Nothing of it goes through the recorder's records or orc_tab_fill_pass.
  oracle side      oracle_tables(): orc_tab_fill_pass on the cu records and the deblocking tu records that recorder_units_cases.expect_units derives, the MvField
                   table of mvf_unit_cases.expect_table on its motion records, the QP tables of qp_rec_cases.expected on its sidecars; then
                   orc_deblock_bs_pass + orc_deblock_frame_pass x 2, orc_sao_frame_pass, orc_alf_frame_pass on the oracle chain's
                   reconstruction (ref_picture_cases.run_oracle).

Drawn per picture, seeded by its place in the list: even per-CTU deblocking offsets in -24..24, reference POC lists with repeats, LADF on for
two pictures in three with bounds from quantiles of the reconstructed luma (the oracle chain's, which ref_picture.json pins to the
reference's, so that the GPU test can draw them without the library), pps_loop_filter_across_slices / _tiles in all four combinations over the
list, SAO / ALF parameters by ref_pass_cases.draw_filter on this picture's geometry, and ONE CTB per picture with SAO, ALF and CC-ALF off.

Domain: ref_picture_cases.in_domain carries over; the tables are on the 4-grid (minimum coding block 4, which the record passes require);
nothing above 264x136; 4:0:0 runs with one component.

Sensitivity (MISREADINGS, each applied to the oracle side or to the derivation of its inputs alone; SENSITIVITY names the listed pictures
that then differ from the reference in a compared table or plane; tests/test_ref_decoded_cpu.py recomputes the table):
  bs_from_refined_motion          boundary strengths from tab_dmvr_mvf instead of the table the parser stored
  ciip_not_strong                 ciip_flag cleared in the table the strength rule reads
  joint_qp_from_cb_cr             the chroma QP of a joint TU with both blocks coded from qp[CB] / qp[CR]
  qp_y_skips_uncoded_units        qp_y not painted for uncoded units (their entries keep the value 0 the table starts with)
  chroma_flag_from_luma_flag      both chroma coded flags of a TU record taken from its luma flag
  no_64_split_of_128              one transform unit for a unit of 128 (no transform edge at 64)
  deblock_before_inverse_lmcs     the filters run on the reconstruction, inverse LMCS applied to what ALF leaves
  sao_after_vertical_only         SAO fed the planes after the vertical pass
  ladf_from_unmapped_luma         the LADF level read from the luma before inverse LMCS.  The oracle's pass reads the level from the plane it
                                  filters, as the reference does, so this one is a MODEL: where the LADF interval of the unmapped luma at a
                                  unit's left edge differs from that of the mapped luma, the difference of the two QP offsets is added to
                                  the unit's qp_y.  Pictures without LADF or without a slice that uses LMCS cannot differ.

The quiet pictures Q0-Q2 exist because W0-W9 carry residuals at QPs up to 74 on steep, noisy content: only the weak luma filter fires there.
They are the same generator's drawings with few coded units, one level of +-1 per coded block at a low QP, a high QP on the units without a
residual (only the deblocking tables read it), gentle reference pictures (Q0, Q2), inter units of 128 (Q0), and neighbours of equal motion
beside DMVR units (_twin_motion).  With them every class of PREMISES is reached: NOT_REACHED is empty.  A class that no decoded picture
reaches would be listed there with the reason (at most two); it would stay covered by D14 and test_deblock_packed_gpu.py.

First run.  The reference and the chain disagreed on three rules of the transform-unit records, and all three times the records were wrong
for deblocking.  (1) No TU record carried the pcm bit, so two neighbouring BDPCM blocks got strength 2 where the reference gives 0.
(2) An ISP unit got one tree-1 record per partition, with the Cb / Cr flags and QPs of partitions that have no chroma, where the
reference has ONE chroma block over the whole unit: chroma edges and chroma QPs inside such units were wrong.  (3) ISP partitions 1 or 2
samples wide got records the device passes skip, which left their 4x4 units without a transform unit.  vvc355_rec_units' list stays as it
was (its callers and their tests depend on it); the recorder now keeps a second list by the reference's rules, vvc355_rec_deblock_units,
and recorder_units_cases.tu_records() states it.  Both sides of this module, and the device test, use that list."""
import ctypes
import json
import os
from collections import Counter
from types import SimpleNamespace

import numpy as np

import bs_cases
import mvf_unit_cases as mu
import qp_rec_cases as qc
import recorder_units_cases as uc
import ref_pass_cases as ps
import ref_picture_cases as pc
import ref_recon_cases as rc
from ffvvc_amd import abi

GOLDEN_PATH = os.path.join(rc.ROOT, "tests", "golden", "ref_decoded.json")
SEED = 0xDEC0DED0
SWEEP = 48
MVF = np.dtype(abi.MvField)
STAGES = ("h", "sao", "alf")

# the quiet pictures (module docstring): name -> (what ref_recon_cases.draw draws, share of CIIP units, slice with explicit weights)
_QUIET = {
    "Q0": (dict(bd=10, idc=1, ctb_log2=7, size=(264, 136), intra=0.1, slices=[(0, 0), (0, 1)], lmcs=True, big_inter=True, inter_ctu=0.6, min_cu=8,
                tools=dict(cu_coded=0.25, coded=0.5, isp=0.0, sbt=0.3)), 0.15, None),
    "Q1": (dict(bd=8, idc=2, ctb_log2=6, size=(200, 136), intra=0.1, slices=[(0, 0)], tiles=True, min_cu=8, inter_ctu=0.5,
                tools=dict(cu_coded=0.25, coded=0.5, isp=0.0)), 0.15, None),
    "Q2": (dict(bd=12, idc=3, ctb_log2=5, size=(136, 104), intra=0.1, slices=[(0, 1), (0, 0)], lmcs=True, min_cu=8, inter_ctu=0.5,
                tools=dict(cu_coded=0.25, coded=0.5, isp=0.0)), 0.15, None),
}
_QUIET_SEED = {"Q0": 22, "Q1": 1, "Q2": 2}       # Q0's is the first offset whose drawing holds coded inter units of 128
_GENTLE = ("Q0", "Q2")                           # gentle reference pictures; Q1 keeps the usual content, on which DMVR refines by whole samples
RASTER_TOO = ("W0", "Q2")                      # the pictures the GPU test also runs with the CTUs in raster ticket order
ENTRIES_TOO = ("W1", "W0", "W5")               # 8 / 10 / 12 bit: also through the separate entries in INTEGRATION.md's order

SENSITIVITY = {
    "bs_from_refined_motion": ["Q1"],
    "ciip_not_strong": ["W0", "W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9", "Q0", "Q1", "Q2"],
    "joint_qp_from_cb_cr": ["W0", "W1", "W2", "W4", "W5", "W6", "W8", "W9", "Q0", "Q1", "Q2"],
    "qp_y_skips_uncoded_units": ["W0", "W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9", "Q0", "Q1", "Q2"],
    "chroma_flag_from_luma_flag": ["W0", "W1", "W2", "W4", "W5", "W6", "W7", "W8", "W9", "Q0", "Q1", "Q2"],
    "no_64_split_of_128": ["Q0"],
    "deblock_before_inverse_lmcs": ["W0", "W1", "W2", "W4", "W5", "W6", "W7", "W9", "Q0", "Q2"],
    "sao_after_vertical_only": ["W0", "W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9", "Q0", "Q1", "Q2"],
    "ladf_from_unmapped_luma": ["W0", "W1", "W4", "W7", "W9", "Q0", "Q2"],
}
MISREADINGS = ("bs_from_refined_motion", "ciip_not_strong", "joint_qp_from_cb_cr", "qp_y_skips_uncoded_units", "chroma_flag_from_luma_flag",
               "no_64_split_of_128", "deblock_before_inverse_lmcs", "sao_after_vertical_only", "ladf_from_unmapped_luma")


def picture_names():
    return pc.picture_names() + list(_QUIET)


# ---------------------------------------------------------------------------------------------------------------- drawing

def _quieten(pic, rng):
    """cu->qp[] feeds both derive_qp (the residual's scale) and the deblocking tables.  A unit that carries a residual gets a LOW QP and one
    level of +-1 at DC per coded block; a unit without any (most of them) gets a HIGH QP, which only the deblocking tables read."""
    off = 6 * (pic.bd - 8)
    for ctu in pic.ctus:
        for cu in ctu:
            coded = bool(cu["coded_flag"]) and any(b["has"] for tu in cu["tus"] for b in tu["tbs"])
            if coded:
                cu["qp"] = [int(rng.integers(4, 13)) - off] + [int(rng.integers(4, 13)) for _ in range(3)]
            else:
                cu["qp"] = [int(rng.integers(40, 58))] + [int(rng.integers(40, 58)) + off for _ in range(3)]
            for tu in cu["tus"]:
                for b in tu["tbs"]:
                    if b["has"]:
                        lv = np.zeros_like(b["levels"])
                        lv[0, 0] = int(rng.choice([-1, 1]))
                        b["levels"], b["nzw"], b["nzh"] = lv, 1, 1
    pic._flat = None
    return pic


def _gentle(rng, h, w, bd, scale=64):
    """bipred_cases.smooth_picture without its noise, on a coarser grid and a sixteenth of the range: the slope is about one level a sample
    at 10 bit and the second differences vanish off the grid lines, so the smoothness decisions of the strong and long filters can pass."""
    gh, gw = h // scale + 2, w // scale + 2
    g = (1 << (bd - 1)) + rng.integers(-(1 << (bd - 5)), (1 << (bd - 5)) + 1, size=(gh, gw)).astype(np.float64)
    ys, xs = np.arange(h) / scale, np.arange(w) / scale
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    p = g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0] * fy * (1 - fx) + g[y0 + 1][:, x0 + 1] * fy * fx
    return np.ascontiguousarray(np.rint(p).astype(rc.px(bd)))


def _quiet_content(k, bd):
    """The content hook of a quiet picture (recorder_chain_cases.content): gentle reference pictures, displaced per list and index as
    ciip_frame_cases.pictures displaces them, and that function's forward map."""
    import bipred_cases as bc

    def content(p):
        rng = np.random.default_rng([SEED, 5, k])
        dims = [(p.width, p.height)] + [(p.width >> p.hs, p.height >> p.vs)] * 2
        base = [_gentle(rng, ph, pw, bd) for (pw, ph) in dims]
        refs = [[[bc.shifted(base[c], (2 * l - 1) * (r + 1) >> (p.hs if c else 0), (1 - 2 * l) * (r + 2) >> (p.vs if c else 0)) for c in range(3)]
                 for r in range(2)] for l in range(2)]
        lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)
        return dims, refs, lut
    return content


def _twin_motion(pic, rng, frac=0.6):
    """Random motion never leaves two neighbours within half a sample of each other, and few units draw DMVR.  Here (i) more of the regular
    units that the parser's rule allows get DMVR, (ii) the inter unit to the right of and the one below a DMVR unit (same CTU, no CIIP
    unit) become regular units WITHOUT DMVR that carry the DMVR unit's unrefined motion, (iii) other regular units take over the motion of
    the regular unit to their left.  Between such neighbours the table the parser stored gives strength 0 — and tab_dmvr_mvf gives
    strength 1 where the refinement reached half a sample."""
    ctb = 1 << pic.ctb_log2
    units = [cu for ctu in pic.ctus for cu in ctu if cu.get("pu") and not cu["ciip_flag"]]
    plain = lambda cu: cu["pu"]["kind"] == mu.PLAIN and not cu["pu"]["msf"]                  # noqa: E731
    for cu in units:
        pu, w, h = cu["pu"], cu["w"], cu["h"]
        m = pu["motion"][:6].view(uc.MVF)[0]
        if plain(cu) and not pu["dmvr"] and int(m["pred_flag"]) == 3 and not int(m["bcw_idx"]) and w >= 8 and h >= 8 and w * h >= 128 and rng.random() < frac:
            nsx, nsy = max(1, w // 16), max(1, h // 16)
            pu.update(dmvr=1, nsx=nsx, nsy=nsy, motion=np.tile(pu["motion"][:6], nsx * nsy).copy())
    taken = set()
    for cu in units:
        if not (plain(cu) and cu["pu"]["dmvr"]) or id(cu) in taken:
            continue
        for x, y in ((cu["x0"] + cu["w"], cu["y0"]), (cu["x0"], cu["y0"] + cu["h"])):
            if x >= pic.width or y >= pic.height or (x // ctb, y // ctb) != (cu["x0"] // ctb, cu["y0"] // ctb):
                continue
            other = pc._unit_at(pic, x, y)
            if other.get("pu") and not other["ciip_flag"] and not (plain(other) and other["pu"]["dmvr"]) and id(other) not in taken:
                other["pu"] = dict(kind=mu.PLAIN, msf=0, nsx=1, nsy=1, dmvr=0, bdof=0, hpel=cu["pu"]["hpel"], bcw=0, pred_flag=0, model=0, part=0, ref_idx=[0, 0],
                                   motion=cu["pu"]["motion"][:6].copy())
                taken.add(id(other))
    for cu in units:
        pu = cu["pu"]
        if id(cu) in taken or not plain(cu) or pu["dmvr"] or pu["bdof"] or not cu["x0"] % ctb or rng.random() >= frac:
            continue
        left = pc._unit_at(pic, cu["x0"] - 1, cu["y0"])
        if left.get("pu") and not left["ciip_flag"] and plain(left):
            pu["motion"], pu["hpel"] = left["pu"]["motion"][:6].copy(), left["pu"]["hpel"]


_pictures = {}


def picture(name):
    if name in _QUIET:
        if name not in _pictures:
            kw, frac, which = _QUIET[name]
            k = list(_QUIET).index(name)
            pic = rc.draw(name, SEED + _QUIET_SEED[name], **kw)
            pic = uc.dress(_quieten(pic, np.random.default_rng([SEED, 3, k])), 9000 + k, frac)
            _twin_motion(pic, np.random.default_rng([SEED, 4, k]))
            if name in _GENTLE:
                pic.content = _quiet_content(k, pic.bd)
            _pictures[name] = pc.finish(pic, np.random.default_rng([SEED, 1, k]), which)
        return _pictures[name]
    return pc.picture(name)


def sweep_picture(k):
    return pc.sweep_picture(k)


# ---------------------------------------------------------------------------------------------------------------- the tables from the units

class UnitTables(bs_cases.BsTables):
    """A BsTables (its arrays, frame() and fill_frame()) without the generator: every table starts from zero, as the reference clears them."""

    def __init__(self, pic, lfase, lfate, ref_poc):
        self.width, self.height, self.ctb_log2 = pic.width, pic.height, pic.ctb_log2
        self.cw, self.ch, self.tw, self.th = pic.ncx, pic.ncy, pic.width // 4, pic.height // 4
        self.lfase, self.lfate, self.hs, self.vs = lfase, lfate, pic.hs, pic.vs
        for n in self.IN:
            if n not in ("mvf", "ref_poc", "slice_idx", "col_bd", "row_bd"):
                setattr(self, n, np.zeros((self.th, self.tw), np.int32 if n in ("tbx0", "tbx1", "tby0", "tby1", "cbx", "cby") else np.uint8))
        self.mvf = np.zeros((self.th, self.tw), MVF)
        self.slice_idx, self.col_bd, self.row_bd, self.ref_poc = pic.slice_idx, pic.col_bd, pic.row_bd, ref_poc


def _blocks(pic, cu, tu):
    """A transform unit's blocks as the reference's parser adds them: the description's, or (a unit without a residual,
    skipped_transform_tree) one uncoded block per component."""
    if tu["tbs"]:
        return tu["tbs"]
    out = [rc._tb(0, tu["x0"], tu["y0"], tu["w"], tu["h"], 0)] if cu["tree_type"] != 2 else []
    if pic.idc and cu["tree_type"] != 1:
        out += [rc._tb(c, tu["x0"], tu["y0"], tu["w"] >> pic.hs, tu["h"] >> pic.vs, 0) for c in (1, 2)]
    return out


def _tb_tab(tab, v, pic, b):
    """set_tb_tab (vvc_ctu.c:62): rows in steps of 4 luma samples, FFMAX(1, width >> 2) entries each."""
    hs, vs = (pic.hs, pic.vs) if b["c_idx"] else (0, 0)
    width, height = b["w"] << hs, b["h"] << vs
    for h in range(0, height, 4):
        tab[(b["y0"] + h) >> 2, (b["x0"] >> 2):(b["x0"] >> 2) + max(1, width >> 2)] = v


def _tb_pos(t, pic, b):
    """set_tb_pos (vvc_ctu.c:41): position in luma samples, size in the component's samples."""
    hs, vs = (pic.hs, pic.vs) if b["c_idx"] else (0, 0)
    tree = int(b["c_idx"] != 0)
    s = np.s_[(b["y0"] >> 2):(b["y0"] >> 2) + max(1, b["h"] >> (2 - vs)), (b["x0"] >> 2):(b["x0"] >> 2) + max(1, b["w"] >> (2 - hs))]
    (t.tbx1 if tree else t.tbx0)[s], (t.tby1 if tree else t.tby0)[s] = b["x0"], b["y0"]
    (t.tbw1 if tree else t.tbw0)[s], (t.tbh1 if tree else t.tbh0)[s] = b["w"], b["h"]


def reference_tables(pic, mvf, lfase, lfate, ref_poc):
    """(UnitTables, {qp_y, qp_c0, qp_c1}) painted straight from the units in decoding order."""
    t = UnitTables(pic, lfase, lfate, ref_poc)
    qp = {k: np.zeros((t.th, t.tw), np.int8) for k in qc.TABLES}
    cbf = (t.cbf0, t.cbf1, t.cbf2)
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] != 2:
                s = np.s_[cu["y0"] >> 2:(cu["y0"] + cu["h"]) >> 2, cu["x0"] >> 2:(cu["x0"] + cu["w"]) >> 2]
                t.cbx[s], t.cby[s], t.cbw[s], t.cbh[s] = cu["x0"], cu["y0"], cu["w"], cu["h"]                  # set_cb_pos
                pu = cu.get("pu")
                t.msf[s], t.iaf[s] = (pu["msf"], int(pu["kind"] == mu.AFFINE)) if pu else (0, 0)             # set_cb_tab
                qp["qp_y"][s] = uc._qp8(cu["qp"][0])                                                          # set_qp_y
            for tu in cu["tus"]:
                both = tu["joint"] and tu["coded"][1] and tu["coded"][2]
                for b in _blocks(pic, cu, tu):
                    c = b["c_idx"]
                    if b["has"]:
                        _tb_tab(cbf[c], tu["coded"][c], pic, b)
                    if c != 2:
                        _tb_pos(t, pic, b)
                    if c == 1:
                        _tb_tab(t.joint, tu["joint"], pic, b)
                    if c:                                                                                      # set_cu_tabs
                        _tb_tab(qp[f"qp_c{c - 1}"], uc._qp8(cu["qp"][3 if both else c]), pic, b)
                    if c != 2 and cu["bdpcm"][c]:
                        _tb_tab(t.pcm1 if c else t.pcm0, 1, pic, b)
    t.mvf[:] = np.ascontiguousarray(mvf).view(MVF).reshape(t.th, t.tw)
    return t, qp


def oracle_tables(orc, pic, e, lfase, lfate, ref_poc, misread=None, dmvr=None):
    """(UnitTables, QP tables) from the records expect_units derives: orc_tab_fill_pass, mvf_unit_cases.expect_table, qp_rec_cases.expected."""
    g = mu.Geo(pic.width, pic.height, pic.ctb_log2)
    t = UnitTables(pic, lfase, lfate, ref_poc)
    cu, tu, cu_qp, tu_qp_c = e.cu.copy(), e.tud.copy(), e.cu_qp.copy(), e.tud_qp_c.copy()         # the deblocking list: vvc355_rec_deblock_units
    tu_first = e.first_tud
    if misread == "chroma_flag_from_luma_flag":
        # a tree-1 record follows the unit's tree-0 records in the same order: pair them by rectangle
        luma = {(int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])): int(r["flags"]) & 1 for r in tu if not r["flags"] & 0x80}
        for r in tu:
            key = (int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"]))
            if r["flags"] & 0x80 and key in luma:
                r["flags"] = (int(r["flags"]) & ~0x06) | (luma[key] << 1) | (luma[key] << 2)
    if misread == "no_64_split_of_128":
        keep = np.ones(len(tu), bool)
        big = {(int(c["x0"]), int(c["y0"])): (int(c["w"]), int(c["h"])) for c in cu if max(int(c["w"]), int(c["h"])) > 64}
        for i, r in enumerate(tu):
            x, y = int(r["x0"]), int(r["y0"])
            for (bx, by), (bw, bh) in big.items():
                if bx <= x < bx + bw and by <= y < by + bh:
                    if (x, y) == (bx, by):
                        tu[i]["w"], tu[i]["h"] = bw, bh
                    else:
                        keep[i] = False
        rs = mu.ctu_of(tu_first, len(tu))
        tu, tu_qp_c = tu[keep], tu_qp_c[keep]
        tu_first = np.searchsorted(rs[keep], np.arange(len(tu_first))).astype(np.int32)
    if misread == "joint_qp_from_cb_cr":
        k = 0
        for ctu in pic.ctus:
            for unit in ctu:
                for tree in range(int(unit["tree_type"] == 2), 1 + int(pic.idc != 0 and unit["tree_type"] != 1)):
                    for _rec in uc.tu_records(pic, unit, tree):
                        if tree:
                            tu_qp_c[k] = (uc._qp8(unit["qp"][1]), uc._qp8(unit["qp"][2]))
                        k += 1
        assert k == len(tu_qp_c)
    if misread == "qp_y_skips_uncoded_units":
        coded = [bool(unit["coded_flag"]) for ctu in pic.ctus for unit in ctu if unit["tree_type"] != 2]
        assert len(coded) == len(cu)
        w = cu["w"].copy()
        w[~np.array(coded)] = 0                                                  # a record that paints nothing
        cu_paint = cu.copy()
        cu_paint["w"] = w
    else:
        cu_paint = cu
    orc.orc_tab_fill_pass.argtypes, orc.orc_tab_fill_pass.restype = [ctypes.POINTER(abi.TabFill)], None
    f = t.fill_frame(cu.ctypes.data if len(cu) else 0, tu.ctypes.data if len(tu) else 0, 0, (len(cu), len(tu), 0), lambda n: getattr(t, n).ctypes.data)
    orc.orc_tab_fill_pass(ctypes.byref(f))
    table = np.zeros((g.th, g.tw), mu.MVF_DT)
    ok = mu.expect_table(g, e.mvf, e.first_mvf, table, len(e.affine))
    assert ok.all(), f"{pic.name}: a motion record the pass would not place"
    if misread == "bs_from_refined_motion":
        table = dmvr.copy()
    if misread == "ciip_not_strong":
        table["ciip_flag"] = 0
    t.mvf[:] = np.ascontiguousarray(table).view(MVF).reshape(t.th, t.tw)
    qp = qc.expected(qc.Pic(g=g, cu=cu_paint, tu=tu, cu_first=e.first_cu, tu_first=tu_first, cu_qp=cu_qp, tu_qp_c=tu_qp_c))
    return t, qp


# ---------------------------------------------------------------------------------------------------------------- one case

_cases = {}


def _index(pic):
    names = picture_names()
    return names.index(pic.name) if pic.name in names else 100 + int(pic.name.rsplit("/", 1)[-1])


def case(orc, pic):
    """Everything the filter half of `pic` is fed, made once: the drawn parameters, the reference side's tables, the oracle side's."""
    key = id(pic)
    if key in _cases:
        return _cases[key]
    i = pc.inputs(pic)
    k = _index(pic)
    rng = np.random.default_rng([SEED, 7, k])
    n_comp = 3 if pic.idc else 1
    lfase, lfate = k & 1, (k >> 1) & 1
    n_sl = len(pic.slices)
    ref_poc = rng.choice(np.array([0, 4, 8], np.int32), size=(n_sl, 2, 32)).astype(np.int32)
    dbp = (2 * rng.integers(-12, 13, size=(pic.ncx * pic.ncy, 6))).astype(np.int8)
    o = pc.run_oracle(orc, pic)
    ladf = None
    if k % 3 != 2:
        bounds = [0] + [int(v) for v in np.quantile(o.final[0], [0.2, 0.4, 0.6, 0.8])]
        for j in range(1, 5):
            bounds[j] = max(bounds[j], bounds[j - 1] + 1)
        ladf = dict(bounds=bounds, lowest=int(rng.integers(-12, 13)), offsets=[int(v) for v in rng.integers(-12, 13, size=4)])
    t_ref, qp_ref = reference_tables(pic, i.mvf, lfase, lfate, ref_poc)
    t_orc, qp_orc = oracle_tables(orc, pic, i.e, lfase, lfate, ref_poc)
    dp_ref = ps._finish_deblock(pic.name, pic.bd, n_comp, t_ref, None, qp_ref, dbp, ladf, None)
    dp_orc = ps._finish_deblock(pic.name, pic.bd, n_comp, t_orc, None, qp_orc, dbp, ladf, None)
    fp = ps.draw_filter(pic.name, rng, pic.bd, (pic.hs, pic.vs), n_comp, pic.ctb_log2, None, n_sl, True, (lfase, lfate), t=t_ref, planes=False)
    quiet = int(rng.integers(0, pic.ncx * pic.ncy))                         # the CTB with SAO, ALF and CC-ALF off
    sao, alf = fp.sao.view(np.dtype(abi.SaoCtb)), fp.alf.view(np.dtype(abi.AlfCtb))
    sao["type_idx"][quiet], alf["ctb_flag"][quiet], alf["cc_idc"][quiet] = 0, 0, 0
    fp.n_slices = n_sl
    c = SimpleNamespace(pic=pic, i=i, k=k, n_comp=n_comp, dp_ref=dp_ref, dp_orc=dp_orc, fp=fp, ladf=ladf, dbp=dbp, quiet=quiet, oracle=o,
                        lfase=lfase, lfate=lfate, ref_poc=ref_poc)
    _cases[key] = c
    return c


# ---------------------------------------------------------------------------------------------------------------- both sides

def _filters(lib, side, dp, fp, planes, sao_from="h"):
    out = ps.run_deblock(lib, side, dp, planes)
    out["sao"] = ps.run_filter(lib, side, fp, "sao", out[sao_from])
    out["alf"] = ps.run_filter(lib, side, fp, "alf", out["sao"])
    for k in qc.TABLES:
        out[k] = dp.arrays[k]
    return out


def run_reference(lib, orc, pic):
    """ref_decode_picture, then the reference's three filter callers on its output with the tables painted from the units: the decode's
    result `r` and {tables, "v", "h", "sao", "alf"}.  A -1 from any entry is an assertion."""
    c = case(orc, pic)
    r = pc.run_reference(lib, pic)
    assert r.ret == 0, f"{pic.name}: ref_decode_picture refused the picture ({r.ret})"
    return r, _filters(lib, "ref", c.dp_ref, c.fp, r.final)


def run_oracle(orc, pic, misread=None):
    """The oracle chain: ref_picture_cases.run_oracle, then the oracle's filter passes on tables from the records."""
    assert misread is None or misread in MISREADINGS
    c = case(orc, pic)
    o, dp = c.oracle, c.dp_orc
    planes, sao_from = o.final, "h"
    if misread in ("bs_from_refined_motion", "ciip_not_strong", "joint_qp_from_cb_cr", "qp_y_skips_uncoded_units", "chroma_flag_from_luma_flag",
                   "no_64_split_of_128"):
        t, qp = oracle_tables(orc, pic, c.i.e, c.lfase, c.lfate, c.ref_poc, misread, o.dmvr)
        dp = ps._finish_deblock(pic.name, pic.bd, c.n_comp, t, None, qp, c.dbp, c.ladf, None)
    if misread == "deblock_before_inverse_lmcs":
        planes = o.recon
    if misread == "sao_after_vertical_only":
        sao_from = "v"
    out = _filters(orc, "orc", dp, c.fp, planes, sao_from)
    if misread == "ladf_from_unmapped_luma" and c.ladf is not None:
        out = _filters_with_ladf_of(orc, c, dp, o)
    if misread == "deblock_before_inverse_lmcs":
        for s in ("v",) + STAGES:
            out[s] = [np.where(o.mask, pic.inv_lut[out[s][0]], out[s][0]).astype(out[s][0].dtype)] + list(out[s][1:])
    return o, out


def _ladf_level(plane, vertical):
    """ladf_level (vvc_filter_template.c): the mean of the four samples p0,0 p0,3 q0,0 q0,3 across the edge of every 4-sample segment,
    for every 4x4 unit: (th, tw) int; entries on the picture's first column / row are not read."""
    p = plane.astype(np.int64)
    if vertical:
        q0, q3 = p[0::4, 0::4], p[3::4, 0::4]
        p0, p3 = np.roll(p, 1, axis=1)[0::4, 0::4], np.roll(p, 1, axis=1)[3::4, 0::4]
    else:
        q0, q3 = p[0::4, 0::4], p[0::4, 3::4]
        p0, p3 = np.roll(p, 1, axis=0)[0::4, 0::4], np.roll(p, 1, axis=0)[0::4, 3::4]
    return (p0 + p3 + q0 + q3) >> 2


def _ladf_offsets(c, luma):
    """The LADF QP offset per 4x4 unit and direction, from `luma` (get_qp_y, vvc_filter.c:829)."""
    out = []
    for vertical in (1, 0):
        level = _ladf_level(luma, vertical)
        off = np.full(level.shape, c.ladf["lowest"], np.int64)
        alive = np.ones(level.shape, bool)
        for j in range(4):
            alive &= level > c.ladf["bounds"][j + 1]
            off = np.where(alive, c.ladf["offsets"][j], off)
        out.append(off)
    return out


def _filters_with_ladf_of(orc, c, dp, o):
    """A MODEL of the misreading, not the misreading itself (the oracle's pass reads the level from the plane it filters, as the reference
    does): where the LADF interval of the unmapped luma at a unit's left edge differs from that of the mapped luma, the difference of the
    two QP offsets is added to the unit's qp_y.  The run then differs from the right one only at edges beside such a unit, which is all the
    table asks; a picture without LADF, or whose slices do not use LMCS, cannot differ."""
    a, b = _ladf_offsets(c, o.recon[0]), _ladf_offsets(c, o.final[0])
    qp = {k: v.copy() for k, v in dp.arrays.items() if k in qc.TABLES}
    delta = (a[0] - b[0]).astype(np.int64)
    qp["qp_y"] = np.clip(qp["qp_y"].astype(np.int64) + delta, -128, 127).astype(np.int8)
    dp2 = ps._finish_deblock(c.pic.name, c.pic.bd, c.n_comp, dp.t, None, qp, c.dbp, c.ladf, None)
    out = _filters(orc, "orc", dp2, c.fp, o.final)
    for k in qc.TABLES:
        out[k] = dp.arrays[k]
    return out


def differences(pic, dp, want, got, label="reference", stages=("v",) + STAGES):
    """One line per table or plane that differs, stage by stage: [] = the two runs are equal."""
    lines = ps.table_differences(dp, want, got, out_tables(dp.n_comp), label=label)
    for k in qc.TABLES[:dp.n_comp]:
        bad = np.argwhere(want[k] != got[k])
        if len(bad):
            b = tuple(bad[0])
            lines.append(f"{pic.name} {k}: {len(bad)} entries differ, first at unit (row, col) {list(map(int, b))}: {label} {want[k][b]}, other side {got[k][b]}")
    for s in stages:
        lines += ps.plane_differences(pic.name, s, want[s], got[s], label=label)
    return lines


# ---------------------------------------------------------------------------------------------------------------- digests

def out_tables(n_comp):
    return [n for n in bs_cases.BsTables.OUT if n_comp == 3 or n in ("bs00", "bs10", "p0", "p1", "q0", "q1")]


def inputs_digest(orc, pic):
    c = case(orc, pic)
    fp = c.fp
    conf = json.dumps([pc.inputs_digest(pic), c.lfase, c.lfate, c.ladf, c.quiet, c.n_comp], sort_keys=True)
    return rc.sha(np.frombuffer(conf.encode(), np.uint8), c.dbp, c.ref_poc, fp.sao, fp.alf, *fp.aps)


def digests(orc, pic, decoded, out):
    """{key: sha256}: inputs; dmvr; the ten bS / length tables and the QP tables; the planes after H, SAO and ALF."""
    c = case(orc, pic)
    rec = {"inputs": inputs_digest(orc, pic), "dmvr": rc.sha(pc.mvf_bytes(decoded.dmvr))}
    rec.update({n: rc.sha(out[n]) for n in out_tables(c.n_comp)})
    rec.update({n: rc.sha(out[n]) for n in qc.TABLES[:c.n_comp]})
    for s in STAGES:
        rec.update({f"{s}{k}": rc.sha(p) for k, p in enumerate(out[s])})
    return rec


def reference_digests(lib, orc, name):
    pic = picture(name)
    r, out = run_reference(lib, orc, pic)
    return digests(orc, pic, r, out)


def oracle_digests(orc, name):
    pic = picture(name)
    o, out = run_oracle(orc, pic)
    return digests(orc, pic, o, out)


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


# ---------------------------------------------------------------------------------------------------------------- what the pictures reach

def _pocs(c, m, rs):
    s = int(c.pic.slice_idx[rs])
    return sorted(int(c.ref_poc[s][l][int(m["ref_idx"][l])]) for l in (0, 1) if (int(m["pred_flag"]) >> l) & 1)


def _segments(plane_shape, ty, tx, vertical, shift_across, shift_along):
    """Sample rows / columns of the segment of unit (ty, tx) in a plane subsampled by the two shifts: (lines along the edge, position across)."""
    if vertical:
        return np.arange((4 * ty) >> shift_along, ((4 * ty + 3) >> shift_along) + 1), (4 * tx) >> shift_across
    return np.arange((4 * tx) >> shift_along, ((4 * tx + 3) >> shift_along) + 1), (4 * ty) >> shift_across


def _reach(changed, lines, pos, vertical, n):
    """Per side, which of the taps p0..p(n-1) / q0..q(n-1) of a segment changed: (bool[n], bool[n])."""
    size = changed.shape[1] if vertical else changed.shape[0]
    cp, cq = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        for out, at in ((cp, pos - 1 - i), (cq, pos + i)):
            if 0 <= at < size:
                out[i] = changed[lines, at].any() if vertical else changed[at, lines].any()
    return cp, cq


def filter_classes(c, want, pre_v, n):
    """The deblocking classes that CHANGED SAMPLES in the reference's run, read off its own planes before and after each direction and its own
    bS / length tables (the taps of two edges never overlap: an edge's reach is bounded by half the smaller block beside it)."""
    pic, t = c.pic, c.dp_ref.t
    ctb = 1 << pic.ctb_log2
    for vertical, pre, post in ((1, pre_v, want["v"]), (0, want["v"], want["h"])):
        bs, lp, lq = want[f"bs{vertical}0"], want[f"p{vertical}"], want[f"q{vertical}"]
        changed = pre[0] != post[0]
        for ty, tx in np.argwhere(bs > 0):
            if (tx if vertical else ty) == 0:
                continue
            hce = not vertical and (4 * ty) % ctb == 0
            wp, wq = int(lp[ty, tx]), int(lq[ty, tx])
            cut = hce and wp > 3
            if cut:
                wp = 3
            lines, pos = _segments(changed.shape, ty, tx, vertical, 0, 0)
            cp, cq = _reach(changed, lines, pos, vertical, 7)
            cp[wp:], cq[wq:] = False, False
            if not (cp.any() or cq.any()):
                continue
            if cp[3:].any() or cq[3:].any():
                n["luma long filter changed samples"] += 1
                n[f"luma long filter of length {max(np.nonzero(cp)[0].max(initial=-1), np.nonzero(cq)[0].max(initial=-1)) + 1 > 5 and 7 or 5} changed samples"] += 1
            elif cp[2] or cq[2]:
                n["luma strong filter changed samples"] += 1
            else:
                n["luma weak filter changed samples"] += 1
            n["horizontal ctu edge: luma len_p cut to 3 on a segment that changed samples"] += bool(cut)
        if c.n_comp < 3:
            continue
        sa, sl = (pic.hs, pic.vs) if vertical else (pic.vs, pic.hs)
        size = t.tbw1 if vertical else t.tbh1
        for comp in (1, 2):
            bs = want[f"bs{vertical}{comp}"]
            changed = pre[comp] != post[comp]
            for ty, tx in np.argwhere(bs > 0):
                across = tx if vertical else ty
                if across == 0 or (4 * across) % (8 << sa):
                    continue
                hce = not vertical and (4 * ty) % ctb == 0
                sp = int(size[ty, tx - 1] if vertical else size[ty - 1, tx])
                sq = int(size[ty, tx])
                big = sp >= 8 and sq >= 8
                lines, pos = _segments(changed.shape, ty, tx, vertical, sa, sl)
                cp, cq = _reach(changed, lines, pos, vertical, 3)
                if not (cp.any() or cq.any()):
                    continue
                if cp[1:].any() or cq[1:].any():
                    assert big, f"{pic.name}: chroma taps beyond p0 / q0 changed beside a block under 8"
                    if hce:
                        assert not cp[1:].any(), f"{pic.name}: more than p0 changed above a horizontal CTU edge"
                        n["horizontal ctu edge: chroma len_p cut to 1 on a segment whose q side went through the strong filter"] += 1
                    else:
                        n["chroma strong filter (three taps, both sides >= 8) changed samples"] += 1
                else:
                    n["chroma weak filter changed samples"] += 1


def _edges(pic):
    """Every 4-sample segment of every left / upper edge of a luma-tree unit: (vertical, ty, tx, unit, the unit on the P side)."""
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] == 2:
                continue
            x0, y0 = cu["x0"], cu["y0"]
            if x0:
                for y in range(y0, y0 + cu["h"], 4):
                    yield 1, y >> 2, x0 >> 2, cu, pc._unit_at(pic, x0 - 1, y)
            if y0:
                for x in range(x0, x0 + cu["w"], 4):
                    yield 0, y0 >> 2, x >> 2, cu, pc._unit_at(pic, x, y0 - 1)


def census(lib, orc, pic, r=None, want=None):
    """{premise: count} from the reference's run ALONE: its tables, its bS / length tables, its planes before and after every stage."""
    c = case(orc, pic)
    if r is None:
        r, want = run_reference(lib, orc, pic)
    t, i, n = c.dp_ref.t, c.i, Counter()
    ctb, ncx = 1 << pic.ctb_log2, pic.ncx
    rs_of = lambda ty, tx: ((4 * ty) >> pic.ctb_log2) * ncx + ((4 * tx) >> pic.ctb_log2)        # noqa: E731
    mvf = i.mvf
    for vertical, ty, tx, cu, pcu in _edges(pic):
        py, px = (ty, tx - 1) if vertical else (ty - 1, tx)
        rq, rp = rs_of(ty, tx), rs_of(py, px)
        if rq != rp and ((pic.slice_idx[rq] != pic.slice_idx[rp] and not c.lfase) or
                         ((pic.col_bd[rq % ncx], pic.row_bd[rq // ncx]) != (pic.col_bd[rp % ncx], pic.row_bd[rp // ncx]) and not c.lfate)):
            continue
        bs = int(want[f"bs{vertical}0"][ty, tx])
        if t.pcm0[ty, tx] and t.pcm0[py, px]:
            n["strength 0 between two bdpcm blocks"] += bs == 0
            continue
        kq, kp = pc._kind(cu), pc._kind(pcu)
        kinds = {kq, kp}
        if "intra" in kinds:
            n["strength 2 at an intra unit"] += bs == 2
        elif kinds == {"ciip"}:
            n["strength 2 at a ciip unit beside another ciip unit"] += bs == 2
        elif "ciip" in kinds:
            n["strength 2 at a ciip unit beside a regular inter unit"] += bs == 2 and any(k.startswith("regular") for k in kinds)
        else:
            coded = bool(t.cbf0[ty, tx] or t.cbf0[py, px])
            if coded:
                n["strength 1 from a coded luma block"] += bs == 1
            else:
                same = _pocs(c, mvf[ty, tx], rq) == _pocs(c, mvf[py, px], rp)
                n["strength 1 from motion: different reference pictures"] += bs == 1 and not same
                n["strength 1 from motion: a difference of half a sample or more"] += bs == 1 and same
                n["strength 0 between units of equal motion"] += bs == 0 and same
            if c.n_comp == 3 and cu["tree_type"] == 0 and (4 * (tx if vertical else ty)) % (8 << (pic.hs if vertical else pic.vs)) == 0:
                bsc = [int(want[f"bs{vertical}{k}"][ty, tx]) for k in (1, 2)]
                joint = bool(t.joint[ty, tx] or t.joint[py, px])
                cc = bool(t.cbf1[ty, tx] or t.cbf1[py, px] or t.cbf2[ty, tx] or t.cbf2[py, px])
                n["strength 1 from a joint cb-cr transform unit"] += joint and 1 in bsc
                n["strength 1 from a coded chroma block only"] += cc and not joint and not coded and 1 in bsc
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] == 2:
                continue
            x0, y0, w, h = cu["x0"], cu["y0"], cu["w"], cu["h"]
            if cu.get("pu") and cu["pu"]["kind"] == mu.AFFINE:
                for x in range(x0 + 8, x0 + w, 8):
                    n["sub-block edge inside an affine unit on the 8-grid"] += bool(want["p1"][y0 >> 2, x >> 2]) and t.tbx0[y0 >> 2, x >> 2] != x
                for y in range(y0 + 8, y0 + h, 8):
                    n["sub-block edge inside an affine unit on the 8-grid"] += bool(want["p0"][y >> 2, x0 >> 2]) and t.tby0[y >> 2, x0 >> 2] != y
            if cu["isp_type"]:
                at = (y0 >> 2, x0 >> 2)
                n["isp unit with partitions 1 or 2 samples wide or high"] += min(cu["tus"][0]["w"], cu["tus"][0]["h"]) < 4 and bool(want["bs10" if x0 else "bs00"][at])
                if c.n_comp == 3 and cu["tree_type"] == 0:
                    n["isp unit whose one chroma block covers the whole unit"] += (int(t.tbw1[at]) << pic.hs, int(t.tbh1[at]) << pic.vs) == (w, h)
            inner = []
            if cu["coded_flag"] and cu["sbt_flag"]:
                inner.append(("sbt", cu["tus"][1]))
            if cu["isp_type"] and cu["tus"][0]["w"] >= 4 and cu["tus"][0]["h"] >= 4:
                inner.append(("isp parts", cu["tus"][1]))
            if max(w, h) == 128 and len(cu["tus"]) > 1:
                inner.append(("the 64-split of a unit of 128", cu["tus"][1]))
            for what, tu in inner:
                vertical = tu["x0"] != x0
                at = (tu["y0"] >> 2, tu["x0"] >> 2)
                n[f"transform edge inside a unit: {what}"] += bool(want[f"p{int(vertical)}"][at])
    # the refined motion would decide differently: the reference's own strength rule on the reference's own tab_dmvr_mvf
    moved = np.abs(r.dmvr["mv"].astype(np.int64) - mvf["mv"]).max(axis=(2, 3)) >= 16
    if moved.any():
        t2 = UnitTables(pic, c.lfase, c.lfate, c.ref_poc)
        for name in t.IN:
            setattr(t2, name, getattr(t, name))
        t2.mvf = np.ascontiguousarray(r.dmvr).view(MVF).reshape(t.th, t.tw).copy()
        dp2 = ps._finish_deblock(pic.name, pic.bd, c.n_comp, t2, None, {k: c.dp_ref.arrays[k] for k in qc.TABLES}, c.dbp, c.ladf, None)
        other = ps.run_deblock(lib, "ref", dp2, r.final)
        for vertical in (0, 1):
            diff = other[f"bs{vertical}0"] != want[f"bs{vertical}0"]
            near = moved | (np.roll(moved, 1, axis=1) if vertical else np.roll(moved, 1, axis=0))
            n["edge at a unit refined by a sample or more where tab_dmvr_mvf would give another strength"] += int((diff & near).sum())
    filter_classes(c, want, r.final, n)
    _census_sao_alf(c, want, n)
    return n


def _ctb_slices(pic, comp):
    ctb = 1 << pic.ctb_log2
    hs, vs = (pic.hs, pic.vs) if comp else (0, 0)
    for rs in range(pic.ncx * pic.ncy):
        rx, ry = rs % pic.ncx, rs // pic.ncx
        yield rs, np.s_[(ry * ctb) >> vs:(min((ry + 1) * ctb, pic.height)) >> vs, (rx * ctb) >> hs:(min((rx + 1) * ctb, pic.width)) >> hs]


def _census_sao_alf(c, want, n):
    pic, fp = c.pic, c.fp
    ncx, ncy = pic.ncx, pic.ncy
    sao, alf = fp.sao.view(np.dtype(abi.SaoCtb)), fp.alf.view(np.dtype(abi.AlfCtb))
    tile = lambda rs: (int(pic.col_bd[rs % ncx]), int(pic.row_bd[rs // ncx]))        # noqa: E731
    quiet_same = True
    for comp in range(c.n_comp):
        ch_sao = want["h"][comp] != want["sao"][comp]
        ch_alf = want["sao"][comp] != want["alf"][comp]
        for rs, s in _ctb_slices(pic, comp):
            rx, ry = rs % ncx, rs // ncx
            if rs == c.quiet:
                quiet_same &= not ch_sao[s].any() and not ch_alf[s].any()
            kind = int(sao["type_idx"][rs][comp])
            if ch_sao[s].any():
                assert kind, f"{pic.name}: SAO changed CTB {rs} of component {comp} with type 0"
                if kind == 1:
                    n["sao band offset changed samples"] += 1
                else:
                    n[f"sao edge class {int(sao['eo_class'][rs][comp])} changed samples"] += 1
                    near = [r2 for r2 in (rs - 1 if rx else -1, rs + 1 if rx + 1 < ncx else -1, rs - ncx if ry else -1, rs + ncx if ry + 1 < ncy else -1) if r2 >= 0]
                    if any(pic.slice_idx[r2] != pic.slice_idx[rs] for r2 in near):
                        n[f"sao edge offset changed samples in a ctb at a slice edge, across-slices flag {'on' if c.lfase else 'off'}"] += 1
                    if any(tile(r2) != tile(rs) for r2 in near):
                        n[f"sao edge offset changed samples in a ctb at a tile edge, across-tiles flag {'on' if c.lfate else 'off'}"] += 1
            if ch_alf[s].any():
                on = int(alf["ctb_flag"][rs][comp])
                if comp == 0:
                    assert on
                    n["alf luma fixed filter set changed samples" if alf["filt_set_idx_y"][rs] < 16 else "alf luma aps filter set changed samples"] += 1
                else:
                    cc = int(alf["cc_idc"][rs][comp - 1])
                    assert on or cc, f"{pic.name}: ALF changed CTB {rs} of component {comp} with everything off"
                    if on:
                        n[f"alf chroma alternative {int(alf['alt_idx'][rs][comp - 1])} changed samples"] += 1
                    if cc and not on:
                        n["cc-alf alone changed samples"] += 1
    n["a ctb with sao, alf and cc-alf off left byte for byte"] += bool(quiet_same)


PREMISES = (["strength 2 at an intra unit", "strength 2 at a ciip unit beside a regular inter unit", "strength 2 at a ciip unit beside another ciip unit",
             "strength 1 from a coded luma block", "strength 1 from a coded chroma block only", "strength 1 from a joint cb-cr transform unit",
             "strength 1 from motion: different reference pictures", "strength 1 from motion: a difference of half a sample or more",
             "strength 0 between units of equal motion", "strength 0 between two bdpcm blocks", "isp unit with partitions 1 or 2 samples wide or high",
             "isp unit whose one chroma block covers the whole unit", "sub-block edge inside an affine unit on the 8-grid",
             "transform edge inside a unit: sbt", "transform edge inside a unit: isp parts", "transform edge inside a unit: the 64-split of a unit of 128",
             "edge at a unit refined by a sample or more where tab_dmvr_mvf would give another strength",
             "luma weak filter changed samples", "luma strong filter changed samples", "luma long filter changed samples",
             "chroma weak filter changed samples", "chroma strong filter (three taps, both sides >= 8) changed samples",
             "horizontal ctu edge: luma len_p cut to 3 on a segment that changed samples",
             "horizontal ctu edge: chroma len_p cut to 1 on a segment whose q side went through the strong filter",
             "sao band offset changed samples"] + [f"sao edge class {k} changed samples" for k in range(4)] +
            [f"sao edge offset changed samples in a ctb at a {e} edge, across-{e}s flag {f}" for e in ("slice", "tile") for f in ("off", "on")] +
            ["alf luma fixed filter set changed samples", "alf luma aps filter set changed samples", "alf chroma alternative 0 changed samples",
             "alf chroma alternative 1 changed samples", "cc-alf alone changed samples", "a ctb with sao, alf and cc-alf off left byte for byte"])
NOT_REACHED = {}

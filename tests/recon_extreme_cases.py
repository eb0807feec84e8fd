"""Directed worst-case pictures for the reconstruction half of the picture chain — the three TB record passes, the chroma scale pass, the
RECON walk and inverse LMCS — pinned to ff_vvc_reconstruct like the pictures of tests/ref_recon_cases.py, whose generator draws them: this
module only sets draw()'s hooks (content=, levels=, units=, modes=, model=, qp_max=, partition=) and copies nothing of it.  Every picture stays inside the
domain ref_recon_cases states (the dequant limits of _level_limit, asserted on every hooked block; no CIIP; no scaling lists; intra units at
most 64), is deterministic and at most 264x136.  tests/golden/ref_recon_extremes.json holds the reference's digests (tools/gen_golden.py),
in ref_recon.json's format.  Used by tests/test_recon_extremes_cpu.py and tests/test_recon_extremes_gpu.py.

What the quiet pictures (smooth planes, Laplace-like levels) never enter and these do:
  * content: planes of 0 and the maximum only — 16x16 cells of rows, columns, checkerboards, period-2 and period-4 stripes, halves, a single
    maximum in zeros and a single zero in maxima (PATTERNS); Cb repeats the luma cell, Cr inverts it, so CCLM sees both signs of `a`, flat
    cells give diff = 0 and half cells the largest diff; or flat 64x64 units of 0 / maximum, so that a unit's luma average selects the first
    and the last used bin of the LMCS model;
  * levels (matched_levels): for a target sample (x, y) of a block every level of the window has one magnitude and the sign of
    M_v[., y] * M_h[., x] (or its inverse), so the first-stage sum of row y and the residual at (x, y) sit on their analytic bounds; the
    magnitudes are +32767 / -32768 (the ends of the packed stream), a value beyond int16 (the block travels as int32) and, every fourth block,
    the quiet draw; LFNST blocks carry all 8 / 16 inputs at one magnitude with the signs of one kernel column.  Transform-skip and BDPCM blocks
    keep the generator's draw (ts_tb_cases has their premises, here they only have to meet the walk), but for one transform-skip block in four
    with two levels beyond int16;
  * the LMCS model (extreme_model): the first used bin holds the smallest legal codeword count (OrgCW >> 3, chroma_scale_coeff 16384), the last
    one the largest ((OrgCW << 3) - 1, chroma_scale_coeff 256, at 8 bit 258);
  * units (checker_units): inter units without residual carry the patterns, intra units beside and below them read them as references;
    modes (cycled_modes) walks the square units through all 67 modes and the chroma units through the three CCLM modes;
  * partition (strip_ctus): two CTUs of X9 are cut into 64x4 and 4x64 inter units, the most oblong blocks of the inter TB pass.

Transforms stay inside int: the first stage sums at most 32 inputs of magnitude 2^range times a matrix entry (< 2^18 * 2880 < 2^31), LFNST
16 inputs times 127; a scaled residual is clipped to bd + 1 bits before it meets a coefficient of at most 16384 (< 2^27)."""
import ctypes
import itertools
import json
import os
import sys
from collections import Counter
from types import SimpleNamespace

import numpy as np

import intra_tb_cases as itc
import levels_cases as lc
import ref_recon_cases as rc
from ffvvc_amd import abi

ROOT = rc.ROOT
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_recon_extremes.json")
SEED = 0x2EC0E000
BEYOND_INT16 = 100000                       # the magnitude of the blocks that must travel as int32 (where the dequant limit allows it)

_tables = np.load(os.path.join(ROOT, "tests", "golden", "tables_values.npz"))


# ---------------------------------------------------------------------------------------------------------------- transform matrices

def _dct2_cos():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_tables
    finally:
        sys.path.pop(0)
    return np.array(gen_tables.dct2_cos_table(), np.int64)


_COS = _dct2_cos()
_matrix = {}


def matrix(t, n):
    """M[k, i]: what input k adds to output i of the n-point inverse transform of type t (0 DCT-2, 1 DST-7, 2 DCT-8), int64.  The 64-point
    DCT-2 reads 32 inputs."""
    if (t, n) not in _matrix:
        if t == 0:
            k, i = np.arange(min(n, 32))[:, None], np.arange(n)[None, :]
            m = _COS[((2 * i + 1) * k * (64 // n)) & 255] if n > 1 else np.array([[64]], np.int64)
        else:
            m = _tables[f"{'dst7' if t == 1 else 'dct8'}_{n}"].astype(np.int64).reshape(n, n)
        _matrix[(t, n)] = m
    return _matrix[(t, n)]


def tr_types(pic, cu, c_idx, w, h):
    """(horizontal, vertical) transform type of a block, derive_transform_type restated for the sign patterns (the hook asserts that it agrees with
    ref_recon_cases.tr_kinds; the premises are counted with the oracle's own derivation)."""
    isp = cu["isp_type"] != 0
    if c_idx or (isp and cu["lfnst_idx"]):
        return 0, 0
    if pic.mts_enabled and (isp or (cu["sbt_flag"] and max(w, h) <= 32) or
                            (not pic.explicit_mts_intra and cu["pred_mode"] == 1 and not cu["lfnst_idx"] and not cu["mip_flag"])):
        if cu["sbt_flag"]:
            return (1 if cu["sbt_horizontal"] or cu["sbt_pos"] else 2), (1 if not cu["sbt_horizontal"] or cu["sbt_pos"] else 2)
        return int(4 <= w <= 16), int(4 <= h <= 16)
    return {0: (0, 0), 1: (1, 1), 2: (2, 1), 3: (1, 2), 4: (2, 2)}[cu["mts_idx"]]


def lfnst_kernel(w, h, mode, lfnst_idx):
    """(m[i, j]: what input i adds to output j of the inverse LFNST, outputs) of a block, by pred_mode_intra after the wide-angle mapping."""
    n = 48 if (w >= 8 and h >= 8) else 16
    tr_set = 1 if mode < 0 else int(_tables["lfnst_tr_set_index"][mode])
    tab = _tables["lfnst_8x8" if n == 48 else "lfnst_4x4"].astype(np.int64).reshape(4, 2, 16, n)
    return tab[tr_set, lfnst_idx - 1], n


# ---------------------------------------------------------------------------------------------------------------- the hooks

def _sgn(v):
    return np.where(np.asarray(v) < 0, -1, 1).astype(np.int64)


def matched_levels():
    """levels= hook: sign-matched levels of one magnitude (see the module's docstring); block k of a picture takes variant k % 4."""
    n = itertools.count()

    def hook(rng, pic, w, h, qp, dep, tsf, bdpcm, vert, lfnst, dct2, lim, cu, c_idx):
        k = next(n)
        variant = k % 4
        if variant == 3 or (tsf and (bdpcm or variant != 2)):
            return None
        big = min(lim, BEYOND_INT16 if variant == 2 else 32767)
        if tsf:                                                   # one transform-skip block in four travels as int32 as well
            c = np.zeros((h, w), np.int32)
            c[0, 0], c[h - 1, w - 1] = big, -big
            return c, w, h
        low = min(lim, big + (variant != 2))                      # -32768 beside +32767 where the limit has room
        turn = -1 if variant == 1 else 1
        c = np.zeros((h, w), np.int64)
        if lfnst:
            mode = 0 if (cu["mip_flag"] and not c_idx) else (cu["mode_c"] if c_idx else cu["mode_y"])
            mode = 0 if mode > 80 else rc.wide_angle(cu["isp_type"] != 0, c_idx, w, h, cu["w"], cu["h"], mode)
            m, outs = lfnst_kernel(w, h, mode, cu["lfnst_idx"])
            col = (5 * k) % outs
            for i, (x, y) in enumerate(itc.DIAG4[:itc.lfnst_nz(w, h)]):
                c[y, x] = turn * _sgn(m[i, col])
        else:
            trh, trv = tr_types(pic, cu, c_idx, w, h)
            assert (trh == 0, trv == 0) == tuple(dct2), "tr_types and ref_recon_cases.tr_kinds disagree"
            mw, mh = min(w, 32 if trh == 0 else 16), min(h, 32 if trv == 0 else 16)
            nzw, nzh = (mw, mh) if (k // 4) % 3 else (max(1, mw // 2), max(1, mh - 1))
            x, y = (7 * k + 3) % w, (5 * k + 1) % h
            c[:nzh, :nzw] = turn * _sgn(matrix(trv, h)[:nzh, y])[:, None] * _sgn(matrix(trh, w)[:nzw, x])[None, :]
        c = np.where(c > 0, big, np.where(c < 0, -low, 0)).astype(np.int32)
        nz = np.nonzero(c)
        return c, int(nz[1].max()) + 1, int(nz[0].max()) + 1

    return hook


def _cell(p, yy, xx):
    """Pattern p on cell-local coordinates: True = the maximum, False = 0."""
    return [np.zeros_like(xx, bool), np.ones_like(xx, bool), (yy & 1) == 1, (xx & 1) == 1, ((xx ^ yy) & 1) == 1, ((yy >> 1) & 1) == 1,
            ((xx >> 1) & 1) == 1, (xx == 5) & (yy == 6), ~((xx == 9) & (yy == 3)), xx < 8, yy < 8, ((xx ^ yy) & 2) == 2][p]


PATTERNS = ["zeros", "maxima", "rows", "columns", "checkerboard", "period-4 rows", "period-4 columns", "single maximum", "single zero",
            "left half", "upper half", "2x2 checkerboard"]


def pattern_planes(salt=0, cell=16):
    """content= hook: cells of `cell` luma samples a side, each with one of PATTERNS; Cb repeats the luma cell's pattern at its own scale, Cr
    inverts it."""
    def content(rng, pic, dims):
        top = (1 << pic.bd) - 1
        out = []
        for c, (dh, dw) in enumerate(dims):
            sw, sh = (cell >> pic.hs, cell >> pic.vs) if (c and pic.idc) else (cell, cell)
            yy, xx = np.mgrid[0:dh, 0:dw]
            which = ((xx // sw) * 5 + (yy // sh) * 7 + salt) % len(PATTERNS)
            lx, ly = (xx % sw) * (cell // sw), (yy % sh) * (cell // sh)             # chroma cells show the luma cell, subsampled
            on = np.zeros((dh, dw), bool)
            for p in range(len(PATTERNS)):
                on |= (which == p) & _cell(p, ly, lx)
            out.append(np.where(on != (c == 2), top, 0))
        return out
    return content


def flat_units(salt=0, size=64):
    """content= hook: flat units of `size` luma samples at 0 or the maximum (a checkerboard of units, shifted by salt); Cb takes the other end of
    the range, Cr the unit's own."""
    def content(rng, pic, dims):
        top = (1 << pic.bd) - 1
        out = []
        for c, (dh, dw) in enumerate(dims):
            sw, sh = (size >> pic.hs, size >> pic.vs) if (c and pic.idc) else (size, size)
            yy, xx = np.mgrid[0:dh, 0:dw]
            on = ((xx // sw + yy // sh + salt) & 1) == 1
            out.append(np.where(on != (c == 1), top, 0))
        return out
    return content


def extreme_model(max_bin=15, min_bin=1):
    """model= hook: bins min_bin..max_bin in use; the first holds OrgCW >> 3 codewords, the last (OrgCW << 3) - 1 — the ends of the legal range —
    and the ones between OrgCW / 2.  chroma_scale_coeff = OrgCW * 2^11 / codewords (no delta), 2^11 for an unused bin."""
    def model(bd):
        org = (1 << bd) // 16
        cw = [0] * 16
        for i in range(min_bin, max_bin + 1):
            cw[i] = org >> 1
        cw[min_bin], cw[max_bin] = org >> 3, (org << 3) - 1
        assert sum(cw) <= (1 << bd) - 1 and all(c == 0 or org >> 3 <= c <= (org << 3) - 1 for c in cw)
        m = abi.LmcsModel()
        for i in range(16):
            m.pivot[i + 1] = m.pivot[i] + cw[i]
            m.chroma_scale_coeff[i] = (org << 11) // cw[i] if cw[i] else 1 << 11
        m.min_bin_idx, m.max_bin_idx = min_bin, max_bin
        assert m.chroma_scale_coeff[min_bin] == 16384 and m.chroma_scale_coeff[max_bin] == (org << 11) // ((org << 3) - 1) <= 258
        return m
    return model


def checker_units():
    """units= hook: the leaves of every CTU alternate between inter units without residual (they carry the starting planes' patterns) and intra
    units (where the format allows one), so intra units read the patterns as references from the left and from above."""
    n = itertools.count()

    def units(pic, rs, x, y, w, h):
        small_c = pic.idc != 0 and ((w >> pic.hs) < 4 or (w >> pic.hs) * (h >> pic.vs) < 16)
        k = next(n)
        return "intra" if (k % 3 and not small_c and w <= 64 and h <= 64) else "skip"
    return units


def skip_ctus(which=(0, 3)):
    """units= hook: the CTUs `which` hold inter units without residual only, so the units right of and below them find the starting planes' flat
    luma as neighbours (the average that selects the model's first or last bin); every other unit keeps its draw."""
    def units(pic, rs, x, y, w, h):
        return "skip" if rs in which else None
    return units


def strip_ctus(rows=(2,), cols=(7,)):
    """partition= and units= hooks for the most oblong blocks: the CTUs `rows` (64x64, inside the picture) are cut into eight 64x4 units above two
    32x32 units, the CTUs `cols` into eight 4x64 units beside two 32x32 units; the strips are inter units (their residual goes to the inter TB
    pass as 1:16 blocks), everything else keeps its draw.  skip: CTUs of inter units without residual, as skip_ctus()."""
    def partition(pic, rs):
        x0, y0 = (rs % pic.ncx) << pic.ctb_log2, (rs // pic.ncx) << pic.ctb_log2
        assert not (rs in rows or rs in cols) or (pic.ctb_log2 == 6 and x0 + 64 <= pic.width and y0 + 64 <= pic.height)
        if rs in rows:
            return [(x0, y0 + 4 * i, 64, 4) for i in range(8)] + [(x0, y0 + 32, 32, 32), (x0 + 32, y0 + 32, 32, 32)]
        if rs in cols:
            return [(x0 + 4 * i, y0, 4, 64) for i in range(8)] + [(x0 + 32, y0, 32, 32), (x0 + 32, y0 + 32, 32, 32)]
        return None

    def units(pic, rs, x, y, w, h, skip=(0, 3)):
        if rs in skip:
            return "skip"
        return "inter" if (rs in rows or rs in cols) and min(w, h) == 4 else None
    return partition, units


def cycled_modes(cclm=True):
    """modes= hook: square luma units walk through modes 0..66 (non-square ones walk through the angular modes in the generator already), chroma
    units through the CCLM modes (every second one; the others keep their draw)."""
    n = itertools.count()

    def modes(pic, cu):
        k = next(n)
        out = {}
        if cu["tree_type"] != 2 and cu["w"] == cu["h"] and not cu["mip_flag"] and not cu["bdpcm"][0]:
            mode = k % 67
            if mode or not cu["ref_idx"]:
                out["mode_y"] = mode
        if cclm and pic.idc and cu["tree_type"] != 1 and not cu["bdpcm"][1] and k % 2:
            out["mode_c"] = 81 + (k // 2) % 3
        return out
    return modes


# ---------------------------------------------------------------------------------------------------------------- the pictures

LOW_QP = 16                                 # |level| of 32767 and beyond stays inside the dequant limit at every bit depth and shape

# name -> (what draw() gets, the hooks by name).  One class each; bit depths, formats and CTU sizes are spread over the list.
_LISTED = {
    # transform, intra_tb: all intra, sign-matched levels on pattern planes, LFNST often, two slices (dep-quant on / off, LMCS on / off)
    "X0": dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), intra=1.0, slices=[(1, 1), (0, 0)], lmcs=True, qp_max=LOW_QP, tools=dict(lfnst=0.5, coded=0.9),
               hooks=dict(content="patterns", levels="matched", model="extreme15")),
    # transform, inter_tb: 8 bit 4:4:4, CTU 32, explicit MTS and SBT, tiles; the batched epilogues on 0 / maximum units with the extreme model
    "X1": dict(bd=8, idc=3, ctb_log2=5, size=(136, 104), intra=0.3, tiles=True, wpp=1, slices=[(0, 1), (1, 1)], lmcs=True, explicit_mts=True, qp_max=LOW_QP,
               tools=dict(sbt=0.4, mts=0.8, coded=0.9, cu_coded=1.0), hooks=dict(content="flat32", levels="matched", model="extreme15", units="skipctus")),
    # range 18 (T2's setting): nothing is eligible for the 16-bit path; CTU 128, 128-wide inter units, 4:2:2, joint Cb-Cr with the sign flag
    "X2": dict(bd=12, idc=2, ctb_log2=7, size=(264, 136), intra=0.35, rbits=18, slices=[(1, 1), (1, 0)], lmcs=True, big_inter=True, inter_ctu=0.4, joint_sign=1,
               qp_max=LOW_QP, tools=dict(coded=0.9, joint=0.5), hooks=dict(content="flat64", levels="matched", model="extreme14")),
    # 4:0:0 with units down to 4x4: ISP parts 1 and 2 wide carrying matched residuals, implicit and explicit MTS
    "X3": dict(bd=10, idc=0, ctb_log2=6, size=(136, 72), intra=0.7, min_cu=4, slices=[(0, 0), (1, 0)], explicit_mts=True, qp_max=LOW_QP,
               tools=dict(isp=0.5, coded=0.9), hooks=dict(content="patterns", levels="matched")),
    # the dual-tree case (T4's setting), collocated chroma: CCLM and LFNST on chroma trees over pattern planes
    "X4": dict(bd=10, idc=1, ctb_log2=6, size=(136, 136), intra=1.0, dual=True, min_cu=4, angular=22, slices=[(1, 1), (0, 0)], lmcs=True, collocated=1, joint_sign=1,
               qp_max=LOW_QP, tools=dict(cclm=0.6, coded=0.5), hooks=dict(content="patterns", levels="matched", model="extreme15", modes="cycled")),
    # intra predictors on 0 / maximum neighbours, 10 bit 4:2:0: carriers without residual, few residuals, reference lines 1 and 2, CCLM
    "X5": dict(bd=10, idc=1, ctb_log2=6, size=(264, 136), slices=[(0, 0)], min_cu=8, qp_max=LOW_QP, joint_sign=1,
               tools=dict(coded=0.15, ref_line=0.6, isp=0.15, mip=0.15, bdpcm=0.05, lfnst=0.1, ts=0.1),
               hooks=dict(content="patterns", levels="matched", units="checker", modes="cycled")),
    # the same at 8 bit 4:4:4 with CTU 32 and units down to 4x4: every MIP size id, ISP in both directions, chroma direct MIP
    "X6": dict(bd=8, idc=3, ctb_log2=5, size=(136, 104), slices=[(0, 0), (1, 0)], min_cu=4, qp_max=LOW_QP,
               tools=dict(coded=0.15, mip=0.45, isp=0.3, ref_line=0.4, bdpcm=0.05, lfnst=0.1, ts=0.1),
               hooks=dict(content="patterns3", levels="matched", units="checker", modes="cycled")),
    # the same at 12 bit 4:2:2 with CTU 128: wide angles on oblong units, CCLM on 4:2:2
    "X7": dict(bd=12, idc=2, ctb_log2=7, size=(264, 136), slices=[(1, 0)], min_cu=8, qp_max=LOW_QP, joint_sign=1,
               tools=dict(coded=0.15, ref_line=0.5, cclm=0.7, mip=0.1, isp=0.1, bdpcm=0.05, lfnst=0.1, ts=0.1),
               hooks=dict(content="patterns5", levels="matched", units="checker", modes="cycled")),
    # CCLM at 8 bit 4:2:0 with collocated chroma, CTU 128, wavefront
    "X8": dict(bd=8, idc=1, ctb_log2=7, size=(200, 136), slices=[(0, 0), (1, 0)], min_cu=8, collocated=1, wpp=1, qp_max=LOW_QP,
               tools=dict(coded=0.15, cclm=1.0, mip=0.1, isp=0.1, bdpcm=0.05, lfnst=0.1, ts=0.1),
               hooks=dict(content="patterns7", levels="matched", units="checker", modes="cycled")),
    # residual add: inter units in and around intra CTUs, all five add forms batched and as RESID commands of the walk, joint with the sign
    # flag, units down to 4x4 (chroma blocks of four samples stay unscaled), flat 0 / maximum units under the extreme model; two CTUs cut
    # into 64x4 and 4x64 inter units (strip_ctus): the most oblong blocks of the inter TB pass
    "X9": dict(bd=10, idc=1, ctb_log2=6, size=(264, 136), intra=0.3, inter_ctu=0.5, min_cu=4, tiles=True, slices=[(1, 1), (0, 1), (1, 0)], lmcs=True,
               joint_sign=1, qp_max=LOW_QP, tools=dict(joint=0.6, coded=0.9, cu_coded=1.0, ts=0.15, sbt=0.1), hooks=dict(content="flat64", levels="matched", model="extreme15", strips=True)),
    # the same without the sign flag at 8 bit 4:2:2, CTU 32 (units of 32), the model's last bin left by the end of the search
    "X10": dict(bd=8, idc=2, ctb_log2=5, size=(136, 104), intra=0.3, inter_ctu=0.4, slices=[(0, 1), (1, 0)], lmcs=True, joint_sign=0, qp_max=LOW_QP,
                tools=dict(joint=0.6, coded=0.9, cu_coded=1.0, ts=0.15), hooks=dict(content="flat32s", levels="matched", model="extreme14")),
    # the two pictures the older job path can express as well (OLD_PATH): one slice, one tile, no joint Cb-Cr, no unit above 64
    "X11": dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), intra=0.4, inter_ctu=0.4, slices=[(1, 1)], lmcs=True, qp_max=LOW_QP,
                tools=dict(joint=0.0, coded=0.9, cu_coded=1.0), hooks=dict(content="flat64s", levels="matched", model="extreme15")),
    "X12": dict(bd=8, idc=2, ctb_log2=5, size=(136, 104), intra=0.5, slices=[(0, 0)], explicit_mts=True, qp_max=LOW_QP,
                tools=dict(joint=0.0, coded=0.9, cu_coded=1.0), hooks=dict(content="patterns", levels="matched")),
}
OLD_PATH = ["X11", "X12"]
RASTER_TOO = ["X5", "X9"]                   # the pictures the GPU test also runs in raster ticket order
UNPACKED_TOO = ["X0", "X9"]                 # ... and with packing off
PREDICTOR_PICTURES = ["X4", "X5", "X6", "X7", "X8"]

_HOOKS = {
    "patterns": lambda: pattern_planes(0), "patterns3": lambda: pattern_planes(3), "patterns5": lambda: pattern_planes(5), "patterns7": lambda: pattern_planes(7),
    "flat64": lambda: flat_units(0, 64), "flat64s": lambda: flat_units(1, 64), "flat32": lambda: flat_units(0, 32), "flat32s": lambda: flat_units(1, 32),
    "matched": matched_levels, "extreme15": lambda: extreme_model(15), "extreme14": lambda: extreme_model(14), "checker": checker_units,
    "cycled": cycled_modes, "skipctus": skip_ctus,
}

_pictures = {}


def picture_names():
    return list(_LISTED)


def picture(name):
    """A listed picture; made once (the hooks count the blocks and units they are asked about), nobody writes to it."""
    if name not in _pictures:
        kw = dict(_LISTED[name])
        named = kw.pop("hooks")
        hooks = {k: _HOOKS[v]() for k, v in named.items() if k != "strips"}
        if named.get("strips"):
            hooks["partition"], hooks["units"] = strip_ctus()
        _pictures[name] = rc.draw(name, SEED + list(_LISTED).index(name), **kw, **hooks)
    return _pictures[name]


def inverse_lut(pic):
    """The inverse-LMCS table of a picture: the inverse of its model's piecewise-linear forward mapping (any table does for the pass; this
    one moves both ends of the range)."""
    n = 1 << pic.bd
    org = n // 16
    lut = np.zeros(n, np.int64)
    piv = [int(v) for v in pic.model.pivot]
    for v in range(n):
        i = max([b for b in range(16) if piv[b] <= v and piv[b + 1] > piv[b]] or [0])
        lut[v] = min(n - 1, i * org + (v - piv[i]) * org // max(1, piv[i + 1] - piv[i]))
    return lut.astype(rc.px(pic.bd))


# ---------------------------------------------------------------------------------------------------------------- int64 restatements

def restate_dequant(pic, s):
    """orc_dequant / the reference's scale_coeff on a spec's levels in int64: (coefficients, how many of them the clip to the transform range
    moved)."""
    tsf = bool(s.get("ts"))
    lw, lh, R = s["lw"], s["lh"], pic.rbits
    rect = 0 if tsf else (lw + lh) & 1
    dep = 0 if tsf else s["dep"]
    q = s["qp"] + dep
    shift = 10 if tsf else pic.bd + rect + (lw + lh) // 2 + 10 - R + dep
    scale = rc.LEVEL_SCALE[rect][q % 6] << (q // 6)
    c = s["c"].astype(np.int64)
    raw = (c * scale * 16 + ((1 << shift) >> 1)) >> shift
    assert np.abs(c * scale * 16).max() + ((1 << shift) >> 1) < 1 << 31, "a level outside the reference's int"
    raw = np.where(c != 0, raw, 0)
    out = np.clip(raw, -(1 << R), (1 << R) - 1)
    return out, int(np.sum(out != raw))


def restate_block(pic, s, trh, trv, first_clip=True):
    """The inverse transform of a spec without LFNST in int64 (vvcdsp.c itx_2d / itx_1d): SimpleNamespace(res, beyond = first-stage values the
    clip moved, on_bound = residual samples equal to the bound the clipped first stage allows at their column, coef_moved).  first_clip=False
    leaves the first-stage clip out (a sensitivity row)."""
    w, h, R, bd = 1 << s["lw"], 1 << s["lh"], pic.rbits, pic.bd
    nzw, nzh = s["nzw"], s["nzh"]
    co, moved = restate_dequant(pic, s)
    lo, hi = -(1 << R), (1 << R) - 1
    out = SimpleNamespace(beyond=0, on_bound=0, coef_moved=moved)
    mh, mv = matrix(trh, w), matrix(trv, h)
    dc_only = trh == 0 and trv == 0 and nzw == 1 and nzh == 1
    if w > 1 and h > 1:
        sh2 = 5 + R - bd
        if w == h and dc_only:
            t = (int(co[0, 0]) * 64 + 64) >> 7
            out.res = np.full((h, w), (t * 64 + (1 << (sh2 - 1))) >> sh2, np.int64)
            return out
        kv, kh = min(nzh, mv.shape[0]), min(nzw, mh.shape[0])
        first = (mv[:kv].T @ co[:kv, :nzw] + 64) >> 7                       # (h, nzw)
        tmp = np.clip(first, lo, hi) if first_clip else first
        out.beyond = int(np.sum(tmp != first)) if first_clip else int(np.sum((first < lo) | (first > hi)))
        second = tmp[:, :kh] @ mh[:kh]                                      # (h, w)
        if not first_clip:                                                  # without the clip the sums leave int32: wrap as a device would
            second = ((second + (1 << 31)) % (1 << 32)) - (1 << 31)
        out.res = (second + (1 << (sh2 - 1))) >> sh2
        if kh > 1:
            top = (np.maximum(mh[:kh] * hi, mh[:kh] * lo).sum(axis=0) + (1 << (sh2 - 1))) >> sh2
            bot = (np.minimum(mh[:kh] * hi, mh[:kh] * lo).sum(axis=0) + (1 << (sh2 - 1))) >> sh2
            out.on_bound = int(np.sum((out.res == top[None, :]) | (out.res == bot[None, :])))
        assert not first_clip or (np.abs(first).max() < 1 << 31 and np.abs(second).max() < 1 << 31), "a sum outside the reference's int"
    else:
        sh = 6 + R - bd
        if dc_only:
            out.res = np.full((h, w), (int(co[0, 0]) * 64 + (1 << (sh - 1))) >> sh, np.int64)
            return out
        if w > 1:
            k = min(nzw, mh.shape[0])
            line = co[0:1, :k] @ mh[:k]
        else:
            k = min(nzh, mv.shape[0])
            line = (mv[:k].T @ co[:k, 0:1])
        out.res = (line + (1 << (sh - 1))) >> sh
    return out


def restate_lfnst_sums(pic, s):
    """The inverse LFNST's sums of an LFNST spec before their clip, int64: (how many the clip to the transform range moves, dequantised inputs
    the dequant clip moved)."""
    w, h, R = 1 << s["lw"], 1 << s["lh"], pic.rbits
    win = dict(s, nzw=4, nzh=4)
    co, moved = restate_dequant(pic, win)
    m, _n = lfnst_kernel(w, h, s["mode"], s["lfnst_idx"])
    nz = itc.lfnst_nz(w, h)
    u = np.array([co[y, x] for (x, y) in itc.DIAG4[:nz]], np.int64)
    v = (u @ m[:nz] + 64) >> 7
    return int(np.sum((v < -(1 << R)) | (v > (1 << R) - 1))), moved


# ---------------------------------------------------------------------------------------------------------------- digests

def reference_digests(lib, name):
    """One picture's record of tests/golden/ref_recon_extremes.json from the reference (ref_recon_cases.reference_digests on this list)."""
    pic = picture(name)
    d = rc.derive(pic)
    ret, planes, scales, twice = rc.run_reference(lib, pic)
    assert ret == 0 and not twice, (name, ret, twice)
    table = None
    if d.tpic.model is not None:
        table = np.zeros((d.tpic.uy, d.tpic.ux), np.int16)
        for (ux, uy) in d.routed:
            table[uy, ux] = scales[(ux * pic.size_y, uy * pic.size_y)]
    return rc.digests(pic, d, planes, table)


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


# ---------------------------------------------------------------------------------------------------------------- what the pictures reach

def unit_census(pic):
    """Counts from the unit description alone: the tools and shapes the intra-predictor class asks for."""
    n = Counter()
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["pred_mode"] != 1:
                n["inter unit without residual"] += not cu["coded_flag"]
                continue
            w, h = cu["w"], cu["h"]
            if cu["tree_type"] != 2:
                if cu["mip_flag"]:
                    size_id = 0 if (w == 4 and h == 4) else 1 if (w == 4 or h == 4 or (w == 8 and h == 8)) else 2
                    n[f"mip size id {size_id} transposed {cu['mip_transposed']}"] += 1
                elif cu["isp_type"]:
                    n["isp " + ("horizontal", "vertical")[cu["isp_type"] - 1]] += 1
                    if cu["isp_type"] == 2 and cu["tus"][0]["w"] < 4:
                        n[f"isp parts {cu['tus'][0]['w']} wide with a residual"] += any(tu["coded"][0] for tu in cu["tus"])
                else:
                    m = cu["mode_y"]
                    n[f"luma mode {m}"] += 1
                    n[f"reference line {cu['ref_idx']}"] += 1
                    if w != h and 2 <= m <= 66 and rc.wide_angle(False, 0, w, h, w, h, m) != m:
                        n["wide angle on an oblong unit"] += 1
            if cu["tree_type"] != 1 and pic.idc and 81 <= cu["mode_c"] <= 83:
                n[f"cclm {cu['mode_c']} format {pic.idc} collocated {pic.collocated if pic.idc == 1 else 0}"] += 1
    return n


UNIT_PREMISES = (["inter unit without residual", "isp horizontal", "isp vertical", "isp parts 1 wide with a residual", "isp parts 2 wide with a residual",
                  "reference line 0", "reference line 1", "reference line 2", "wide angle on an oblong unit"] +
                 [f"luma mode {m}" for m in range(67)] +
                 [f"mip size id {i} transposed {t}" for i in range(3) for t in (0, 1)] +
                 [f"cclm {m} format {f} collocated {c}" for m in (81, 82, 83) for (f, c) in ((1, 0), (1, 1), (2, 0), (3, 0))])


def _scaled(v, scale, bd):
    """lmcs_scale_chroma on int64: the residual clipped to bd + 1 bits, times the unit's scale, rounded on the magnitude."""
    v = np.clip(v, -(1 << bd), (1 << bd) - 1)
    return np.sign(v) * ((np.abs(v) * scale + (1 << 10)) >> 11)


def _joint(v, joint):
    return (v * (-1 if joint & 2 else 1)) >> ((joint >> 2) & 1)


def _form(joint):
    return ("scaled " if joint & 8 else "") + (f"joint sign {'-' if joint & 2 else '+'} shift {(joint >> 2) & 1}" if joint & 1 else "" if joint & 8 else "plain")


def inter_workgroup_blocks(lw, lh):
    """Blocks one workgroup of the inter TB pass's shape kernels takes: one lane per 4x4 tile, 256 lanes (itx_shape_body.inc: TBS = 256 / NT)."""
    return max(1, 256 // max(1, (1 << (lw + lh)) // 16))


def census(orc, pic, d, planes, arena):
    """Counts of what the directed pictures are for, from int64 restatements (the transform chain of every block, the residual add of every
    block) and from the oracle side's run (planes, arena: what oracle_side(orc, d) returned).  The transform types are the oracle's own
    derivation; every restated residual must equal the oracle's."""
    import inter_tb_cases as tc
    import ts_tb_cases as ts
    rc.bind_oracle(orc)
    n = Counter()
    bd, top = pic.bd, (1 << pic.bd) - 1
    n_i, n_e = len(d.intra), len(d.inter)
    stream, lv = lc.pack_all([s["c"] for s in d.specs])
    for i, s in enumerate(d.specs):
        name = "intra_tb" if i < n_i else "inter_tb" if i < n_i + n_e else "ts_tb"
        c = s["c"]
        is32 = bool(lv[i]["flags"] & abi.LEVELS_INT32)
        assert is32 == bool(c.max() > 32767 or c.min() < -32768), "a block flagged int32 for another reason than a level beyond int16"
        n[f"{name}: a block that travels as int32"] += is32
        n[f"{name}: +32767 in the packed stream"] += (not is32) and bool((c == 32767).any())
        n[f"{name}: -32768 in the packed stream"] += (not is32) and bool((c == -32768).any())
        if name == "ts_tb":
            continue
        w, h = 1 << s["lw"], 1 << s["lh"]
        off = d.off_of[s["rid"]] if s.get("keep", True) else None       # an intra block always leaves its residual in the arena
        if s.get("lfnst"):
            beyond, moved = restate_lfnst_sums(pic, s)
            size = "4x4" if min(w, h) == 4 else "8x8"
            n[f"lfnst {size} kernel: a sum beyond the range before its clip"] += beyond > 0
            n[f"{name}: a dequantised coefficient on the clip bound"] += moved > 0
            continue
        t = orc.orc_derive_transform_type(s["tu_flags"], s["mts_idx"], s.get("lfnst_idx", 0), s["c_idx"], w, h)
        trh, trv = t & 15, t >> 4
        r = restate_block(pic, s, trh, trv)
        want = itc.oracle_block(orc, s, bd, pic.rbits) if name == "intra_tb" else ts.residual_of(orc, s, bd, pic.rbits)
        assert np.array_equal(r.res.reshape(h, w), np.asarray(want).reshape(h, w)), f"{pic.name}: the int64 restatement of a {w}x{h} block differs from the oracle"
        if off is not None:
            assert np.array_equal(arena[off:off + w * h], r.res.ravel())
        kinds = "DCT-2 DST-7 DCT-8".split()
        shape = "square" if w == h else "oblong 1:%d" % (max(w, h) // min(w, h))
        if r.beyond:
            n[f"{name}: first-stage sums beyond the range before the clip"] += 1
            n[f"{name}: first stage beyond the range, {kinds[trh]} x {kinds[trv]}"] += 1
            n[f"{name}: first stage beyond the range, {shape}"] += 1
            n[f"{name}: first stage beyond the range, 64-point with zero-out"] += max(w, h) == 64
        n[f"{name}: a residual on its bound"] += r.on_bound > 0
        n[f"{name}: a dequantised coefficient on the clip bound"] += r.coef_moved > 0
    # packed records beside int32 records in one workgroup's worth of records of the inter TB pass: the records of a bin are consecutive
    # (inter_tb_cases.group), a shape kernel's workgroup takes inter_workgroup_blocks() of them from the bin's first on
    for ch in range(2):
        for b in range(tc.NB - 1):
            first, last = d.bin_first[ch][b], d.bin_first[ch][b + 1]
            if last > first:
                per = inter_workgroup_blocks(d.inter[first]["lw"], d.inter[first]["lh"])
                for g in range(first, last, per):
                    fl = [bool(lv[n_i + k]["flags"] & abi.LEVELS_INT32) for k in range(g, min(g + per, last))]
                    n["inter_tb: packed beside int32 records in one workgroup"] += any(fl) and not all(fl)
    n["nothing eligible for the 16-bit path (range above 15)"] += pic.rbits > 15 and n_e > 0
    # the residual add: batched epilogues from the starting planes (exact), RESID commands of the walk by |residual| alone (certain)
    table = None
    if d.tpic.model is not None:
        table = np.zeros(d.tpic.ux * d.tpic.uy, np.int16)
        luma = np.ascontiguousarray(planes[0])
        f = rc.scale_frame(pic, luma.ctypes.data, luma.strides[0], table.ctypes.data, ctypes.addressof(pic.model), pic.slice_idx.ctypes.data,
                           pic.col_bd.ctypes.data, pic.row_bd.ctypes.data)
        orc.orc_lmcs_vpdu_scale_pass(bd, ctypes.byref(f))
        table = table.reshape(d.tpic.uy, d.tpic.ux)
    m = pic.model
    ends = {int(m.chroma_scale_coeff[m.min_bin_idx]): "first used bin (largest chroma_scale_coeff)",
            int(m.chroma_scale_coeff[min(m.max_bin_idx + 1, 15)]): "search left behind the last used bin",
            int(m.chroma_scale_coeff[m.max_bin_idx]): "last used bin (smallest chroma_scale_coeff)"} if table is not None else {}

    def tally(where, joint, r, start, wid):
        form = _form(joint)
        lo, hi = (r < -top, r > top) if start is None else (start + r < 0, start + r > top)
        n[f"{where}, {form}: below 0"] += int(lo.sum())
        n[f"{where}, {form}: above the maximum"] += int(hi.sum())
        if start is not None:
            n[f"{where}: overshoot on a starting sample of 0 or the maximum"] += int((lo & (start == 0)).sum() + (hi & (start == top)).sum())
        if wid <= 2:
            n[f"{where}: a block {wid} wide overshoots"] += int(lo.sum() + hi.sum()) > 0
        n["_lo"] += int(lo.sum())
        n["_hi"] += int(hi.sum())

    for s in d.specs[n_i:]:
        if s["keep"]:
            continue
        w, h, c = 1 << s["lw"], 1 << s["lh"], s["c_idx"]
        res = np.asarray(ts.residual_of(orc, s, bd, pic.rbits)).reshape(h, w).astype(np.int64)
        for (plane, joint) in [(c, s["joint"] & 8)] + ([(3 - c, s["joint"])] if s["joint"] & 1 else []):
            r = _joint(res, joint) if joint & 1 else res
            if joint & 8:
                ux, uy = d.tpic.unit_of(s, "cu")
                sc = int(table[uy, ux])
                r = _scaled(r, sc, bd)
                n[f"batched scaled add, {ends.get(sc, 'a bin between')}"] += 1
                n["scaled residual of magnitude 2^bd times the largest coefficient"] += bool(sc == 16384 and (np.abs(r) >= (1 << bd) * 8 - 8).any())
            start = pic.planes[plane][s["y0"]:s["y0"] + h, s["x0"]:s["x0"] + w].astype(np.int64)
            tally("batched", joint, r, start, w)
    for cmd in d.cmds[d.cmds["kind"] == abi.RECON_RESID]:
        w, h, c, joint = int(cmd["w"]), int(cmd["h"]), int(cmd["c_idx"]), int(cmd["joint"])
        off = d.off_of[int(cmd["resid"])]
        r = arena[off:off + w * h].reshape(h, w).astype(np.int64)
        r = _joint(r, joint) if joint & 1 else r
        if joint & 8:
            sc = int(table[int(cmd["cu_y0"]) // pic.size_y, int(cmd["cu_x0"]) // pic.size_y])
            r = _scaled(r, sc, bd)
            n[f"walk scaled add, {ends.get(sc, 'a bin between')}"] += 1
        tally("walk", joint, r, None, w)
    n["reconstruction clips at 0"], n["reconstruction clips at the maximum"] = n.pop("_lo"), n.pop("_hi")
    return n


PASS_PREMISES = [f"{p}: {what}" for p in ("intra_tb", "inter_tb") for what in
                 ("first-stage sums beyond the range before the clip", "a residual on its bound", "a dequantised coefficient on the clip bound",
                  "a block that travels as int32", "+32767 in the packed stream", "-32768 in the packed stream",
                  "first stage beyond the range, square", "first stage beyond the range, oblong 1:8", "first stage beyond the range, oblong 1:16",
                  "first stage beyond the range, 64-point with zero-out")]
PREMISES = (PASS_PREMISES +
            ["ts_tb: a block that travels as int32", "inter_tb: packed beside int32 records in one workgroup", "nothing eligible for the 16-bit path (range above 15)",
             "lfnst 4x4 kernel: a sum beyond the range before its clip", "lfnst 8x8 kernel: a sum beyond the range before its clip"] +
            [f"{p}: first stage beyond the range, {k}" for p, ks in (("intra_tb", ("DCT-2 x DCT-2", "DST-7 x DST-7", "DCT-8 x DCT-8", "DST-7 x DCT-8", "DCT-8 x DST-7",
                                                                                   "DCT-2 x DST-7", "DST-7 x DCT-2")),
                                                                     ("inter_tb", ("DCT-2 x DCT-2", "DST-7 x DST-7", "DCT-8 x DCT-8", "DST-7 x DCT-8", "DCT-8 x DST-7")))
             for k in ks] +
            [f"{where}, {form}: {end}" for where in ("batched", "walk") for end in ("below 0", "above the maximum")
             for form in ("plain", "joint sign + shift 0", "joint sign + shift 1", "joint sign - shift 0", "joint sign - shift 1", "scaled ",
                          "scaled joint sign + shift 0", "scaled joint sign + shift 1", "scaled joint sign - shift 0", "scaled joint sign - shift 1")] +
            ["batched: overshoot on a starting sample of 0 or the maximum", "walk: a block 1 wide overshoots", "walk: a block 2 wide overshoots",
             "batched scaled add, first used bin (largest chroma_scale_coeff)", "batched scaled add, last used bin (smallest chroma_scale_coeff)",
             "batched scaled add, search left behind the last used bin", "walk scaled add, first used bin (largest chroma_scale_coeff)",
             "walk scaled add, last used bin (smallest chroma_scale_coeff)", "scaled residual of magnitude 2^bd times the largest coefficient"])


# ---------------------------------------------------------------------------------------------------------------- sensitivity

# Narrowings a kernel could have, applied to the oracle side's Python glue alone (ref_recon_cases.MISREADINGS' pattern): which listed pictures
# then no longer hash to the reference's digests, here and among T0-T9 of ref_recon_cases (test_recon_extremes_cpu.py recomputes both rows).
# DESIGN.md section 2 has the rows of the narrowings that need an edit of oracle/*.c (observed once, on a copy).
NARROWINGS = ("no_first_stage_clip", "int32_levels_read_as_int16", "residual_held_in_int16", "scaled_product_in_16_bits")
_ALL_X, _ALL_T = [f"X{i}" for i in range(13)], [f"T{i}" for i in range(10)]
SENSITIVITY = {                             # narrowing: (listed pictures here that differ, pictures of T0-T9 that differ)
    "no_first_stage_clip": (_ALL_X, _ALL_T),                             # the quiet pictures reach this clip as well: their levels go up to 14 bits
    "int32_levels_read_as_int16": (_ALL_X, []),                          # only this list has a level beyond int16
    "residual_held_in_int16": (["X0", "X2", "X4", "X5", "X7", "X9", "X11"], ["T2", "T6"]),
    "scaled_product_in_16_bits": (["X1", "X2", "X9", "X10", "X11"], ["T1", "T2", "T5", "T6", "T8"]),
}

# What the issue of this list asked for and the domain does not hold, with the reason (DESIGN.md section 2 repeats it):
UNREACHABLE = {
    "a block eligible for the 16-bit transform path beside an ineligible one in one workgroup":
        "the record passes always dequantise, and the dequantised coefficient is clipped to log2_transform_range bits (Dequant::apply and "
        "apply_small both end in clip_intp2(..., range)) before the eligibility test reads it (itx_shape_body.inc:104-119, mag >> 15; the other "
        "terms at :44-48 hold for every legal record), so at range <= 15 every block is eligible and at range > 15 none is; a coefficient "
        "beyond 16 bits exists only on the older job path with dequantisation off (tests/test_itx_levels_gpu.py).  What the list does reach is "
        "packed records beside int32 records in one workgroup's worth of records, and a whole picture at range 18",
    "a residual of +-2^15 times the largest chroma_scale_coeff":
        "lmcs_scale_chroma clips the residual to bd + 1 bits before the product; the list reaches +-2^bd times 16384",
}


def neighbour_census(pic, d, planes):
    """Per predictor of the walk: luma PRED / CCLM commands whose row above and column to the left (final planes of the oracle side: both are
    complete before the block is predicted) hold 0 and the maximum at once, and commands whose neighbours are flat (CCLM: diff = 0)."""
    n = Counter()
    top = (1 << pic.bd) - 1
    for c in d.cmds:
        kind, c_idx = int(c["kind"]), int(c["c_idx"])
        if kind not in (abi.RECON_PRED, abi.RECON_CCLM) or (kind == abi.RECON_PRED and c_idx):
            continue
        x0, y0, w, h = (int(c[k]) for k in ("x0", "y0", "w", "h"))
        near = np.concatenate([planes[0][y0 - 1, x0:x0 + w] if y0 else [], planes[0][y0:y0 + h, x0 - 1] if x0 else []]).astype(np.int64)
        if not len(near):
            continue
        mode = int(c["mode"])
        tool = ("cclm" if kind == abi.RECON_CCLM else "mip" if c["is_mip"] else "planar" if mode == 0 else "dc" if mode == 1 else
                "horizontal / vertical" if mode in (18, 50) else "angular")
        if tool == "angular" and c["ref_idx"]:
            tool += f", reference line {int(c['ref_idx'])}"
        if c["isp_split"] and kind == abi.RECON_PRED:
            tool += ", isp"
        n[f"{tool}: 0 and the maximum among the neighbours"] += bool((near == 0).any() and (near == top).any())
        n[f"{tool}: flat neighbours"] += bool(near.min() == near.max())
    return n


NEIGHBOUR_PREMISES = ([f"{t}: 0 and the maximum among the neighbours" for t in
                       ("planar", "dc", "horizontal / vertical", "angular", "angular, reference line 1", "angular, reference line 2", "angular, isp", "mip", "cclm")] +
                      ["cclm: flat neighbours"])


def narrowed_oracle_side(orc, d, narrowing):
    """oracle_side(orc, d)'s planes with one of NARROWINGS applied:
      no_first_stage_clip          the blocks without LFNST take restate_block(first_clip=False), wrapped to int32, for their residual;
      int32_levels_read_as_int16   every block's levels are read through int16 (what a packed reader does to a record that should have
                                   travelled as int32);
      residual_held_in_int16       every block's residual wraps to int16 before it is added or handed to the walk;
      scaled_product_in_16_bits    the batched scaled add (orc_lmcs_chroma_resid_block, replaced here by its restatement) holds |residual| *
                                   scale in int16 before the rounding shift."""
    import copy
    import ts_tb_cases as ts
    assert narrowing in NARROWINGS
    pic, bd = d.pic, d.pic.bd
    rc.bind_oracle(orc)
    if narrowing == "int32_levels_read_as_int16":
        d2 = copy.copy(d)
        narrow = lambda s: dict(s, c=s["c"].astype(np.int16).astype(np.int32))                         # noqa: E731
        d2.intra, d2.inter, d2.skip = ([narrow(s) for s in part] for part in (d.intra, d.inter, d.skip))
        d2.specs = d2.intra + d2.inter + d2.skip
        return rc.oracle_side(orc, d2)[0]
    if narrowing == "residual_held_in_int16":
        keep = (itc.oracle_block, ts.residual_of)
        wrapped = [lambda *a, f=f: np.ascontiguousarray(np.asarray(f(*a)).astype(np.int16).astype(np.int32)) for f in keep]
        try:
            itc.oracle_block, ts.residual_of = wrapped
            return rc.oracle_side(orc, d)[0]
        finally:
            itc.oracle_block, ts.residual_of = keep
    if narrowing == "no_first_stage_clip":
        keep = (itc.oracle_block, ts.residual_of)

        def unclipped(orc_, s, bd_, rbits=15):
            if s.get("lfnst") or s.get("ts"):
                return (keep[0] if "cls" in s else keep[1])(orc_, s, bd_, rbits)
            w, h = 1 << s["lw"], 1 << s["lh"]
            t = orc_.orc_derive_transform_type(s["tu_flags"], s["mts_idx"], s.get("lfnst_idx", 0), s["c_idx"], w, h)
            return np.ascontiguousarray(restate_block(pic, s, t & 15, t >> 4, first_clip=False).res.reshape(h, w).astype(np.int32))
        try:
            itc.oracle_block, ts.residual_of = unclipped, unclipped
            return rc.oracle_side(orc, d)[0]
        finally:
            itc.oracle_block, ts.residual_of = keep

    def resid_block_16(bd_, jref, mref):
        j = jref._obj
        res = np.ctypeslib.as_array(ctypes.cast(j.resid, ctypes.POINTER(ctypes.c_int32)), (j.h, j.w)).astype(np.int64)
        assert j.joint & 16
        scale = int(ctypes.c_int16.from_address(j.luma).value)
        r = _joint(res, j.joint) if j.joint & 1 else res
        v = np.clip(r, -(1 << bd_), (1 << bd_) - 1)
        prod = (np.abs(v) * scale).astype(np.int16).astype(np.int64)
        r = np.sign(v) * ((prod + (1 << 10)) >> 11)
        t = ctypes.c_uint8 if bd_ == 8 else ctypes.c_uint16
        for y in range(j.h):
            row = np.ctypeslib.as_array((t * j.w).from_address(j.dst + y * j.dst_stride))
            row[:] = np.clip(row.astype(np.int64) + r[y], 0, (1 << bd_) - 1)
    real = orc.orc_lmcs_chroma_resid_block
    try:
        orc.orc_lmcs_chroma_resid_block = resid_block_16
        return rc.oracle_side(orc, d)[0]
    finally:
        orc.orc_lmcs_chroma_resid_block = real


def predictor_overshoot_census(orc, pic, d, planes):
    """Predicted samples that leave the sample range before a clip, from the oracle's own predictor run with headroom: every PRED command of
    the walk is predicted once more by orc_intra_pred_flat at bit depth bd + 2 on the final planes (the block's neighbours as the walk saw
    them) with every sample raised by O = 2^(bd+1) - 2^(bd-1).  The predictors are exact under that offset — filter taps sum to a power of
    two, PDPC and MIP work on differences, and 2^(bd'-1) = 2^(bd-1) + O keeps MIP's and the no-neighbour default's constant in place — and
    nothing can reach the wider clip, so an output outside [O, O + maximum] is a value the real run had to clip.  Planar, DC and chroma
    interpolation are convex and must never leave the range (asserted: the method's own check); what is counted, separately below 0 and above
    the maximum: `cubic filter` (angular luma blocks; angular PDPC is convex, it only pulls the filter's overshoot inward), `PDPC gradient`
    (modes 18 / 50 with PDPC, the one PDPC form that is not convex) and `MIP`.  12-bit pictures have no headroom run (the oracle's predictors
    exist for 8, 10 and 12 bit).  On every picture, 12-bit ones included, the oracle's own decisions per predicted block are counted as
    well: PDPC on / off by mode class (orc_intra_need_pdpc) and the [1 2 1] reference filter on / off for planar and angular luma blocks
    (orc_intra_ref_filter_flag and the size / reference-line / ISP conditions of orc_intra_pred_flat)."""
    n = Counter()
    if not len(d.order):
        return n
    headroom = pic.bd != 12
    orc.orc_intra_ref_filter_flag.argtypes = [ctypes.c_int]
    orc.orc_intra_ref_filter_flag.restype = ctypes.c_int
    orc.orc_recon_debug_job.argtypes = [ctypes.POINTER(abi.ReconFrame), ctypes.c_int, ctypes.c_int, ctypes.POINTER(abi.IntraJob)]
    orc.orc_recon_debug_job.restype = None
    orc.orc_intra_pred_flat.argtypes = [ctypes.c_int, ctypes.c_void_p]
    orc.orc_intra_pred_flat.restype = None
    orc.orc_intra_need_pdpc.argtypes = [ctypes.c_int] * 5
    orc.orc_intra_need_pdpc.restype = ctypes.c_int
    bd2, top = pic.bd + 2, (1 << pic.bd) - 1
    off = (1 << (bd2 - 1)) - (1 << (pic.bd - 1)) if headroom else 0
    raised = [np.ascontiguousarray(p.astype(np.uint16) + off) for p in planes]
    cmds = np.ascontiguousarray(d.cmds)
    f = rc.recon_frame(pic, d, [p.ctypes.data for p in raised], [p.strides[0] for p in raised], cmds.ctypes.data, d.ctus.ctypes.data, d.order.ctypes.data, 0,
                       pic.slice_idx.ctypes.data, pic.col_bd.ctypes.data, pic.row_bd.ctypes.data, ctypes.addressof(pic.model))
    for rs in d.order:
        first, count = int(d.ctus[rs]["first_cmd"]), int(d.ctus[rs]["n_cmd"])
        for k in range(count):
            if int(cmds[first + k]["kind"]) != abi.RECON_PRED:
                continue
            j = abi.IntraJob()
            orc.orc_recon_debug_job(ctypes.byref(f), int(rs), k, ctypes.byref(j))
            c = int(j.c_idx)
            assert j.plane == raised[c].ctypes.data and j.stride == raised[c].strides[0]
            mode = int(j.mode)
            pdpc = bool(orc.orc_intra_need_pdpc(j.w, j.h, j.bdpcm_flag, mode, j.ref_idx))
            cls = "mip" if j.is_mip else "planar" if mode == 0 else "dc" if mode == 1 else "horizontal / vertical" if mode in (18, 50) else "angular"
            if not j.is_mip:
                n[f"PDPC {'on' if pdpc else 'off'}: {cls}"] += 1
                if c == 0 and cls in ("planar", "angular"):
                    smooth = bool(orc.orc_intra_ref_filter_flag(mode)) and not j.ref_idx and j.w * j.h > 32 and not j.isp_split
                    n[f"[1 2 1] reference filter {'on' if smooth else 'off'}: {cls}"] += 1
            if not headroom:
                continue
            work = raised[c].copy()
            j.plane = work.ctypes.data
            orc.orc_intra_pred_flat(bd2, ctypes.addressof(j))
            out = work[j.y:j.y + j.h, j.x:j.x + j.w].astype(np.int64) - off
            lo, hi = int((out < 0).sum()), int((out > top).sum())
            if j.is_mip:
                tool = "MIP"
            elif mode in (18, 50) and pdpc:
                tool = "PDPC gradient"
            elif mode not in (0, 1, 18, 50) and c == 0:
                tool = "cubic filter"
            else:
                assert lo == hi == 0, f"{pic.name}: a convex predictor (mode {mode}, component {c}) left the range in the headroom run"
                continue
            n[f"{tool}: predicted blocks"] += 1
            n[f"{tool}: samples below 0 before the clip"] += lo
            n[f"{tool}: samples above the maximum before the clip"] += hi
    return n


OVERSHOOT_PREMISES = ([f"{t}: samples {e} before the clip" for t in ("cubic filter", "PDPC gradient", "MIP") for e in ("below 0", "above the maximum")] +
                      [f"PDPC {o}: {c}" for o in ("on", "off") for c in ("planar", "dc", "horizontal / vertical", "angular")] +
                      [f"[1 2 1] reference filter {o}: {c}" for o in ("on", "off") for c in ("planar", "angular")])


class CclmStats(ctypes.Structure):
    """Mirror of the oracle's orc_cclm_stats."""
    _fields_ = [(n, ctypes.c_int64) for n in ("blocks", "diff0", "a_pos15", "a_neg15", "k_is_1", "a_max", "a_min", "below0", "above_max")]


def cclm_census(orc, pic, d):
    """What CCLM's derivation and linear model reach in the picture's walk, from the oracle's own run (orc_cclm_debug_stats: counted inside
    orc_intra_cclm_pred_flat while the oracle side runs; its outputs are the ones the digests pin), keyed by chroma format and `collocated`."""
    orc.orc_cclm_debug_stats.argtypes = [ctypes.c_void_p]
    orc.orc_cclm_debug_stats.restype = None
    st = CclmStats()
    try:
        orc.orc_cclm_debug_stats(ctypes.addressof(st))
        rc.oracle_side(orc, d)
    finally:
        orc.orc_cclm_debug_stats(None)
    n = Counter()
    key = f"cclm format {pic.idc} collocated {pic.collocated if pic.idc == 1 else 0}"
    if st.blocks:
        n[f"{key}: blocks"] = st.blocks
        n[f"{key}: the diff = 0 branch"] = st.diff0
        n[f"{key}: a = +15, its largest value"] = st.a_pos15
        n[f"{key}: a = -15, its smallest value"] = st.a_neg15
        n[f"{key}: samples below 0 before the clip"] = st.below0
        n[f"{key}: samples above the maximum before the clip"] = st.above_max
        n["cclm: k = 1, the smallest shift"] = st.k_is_1
        assert -15 <= st.a_min and st.a_max <= 15
    return n


CCLM_PREMISES = ([f"cclm format {f} collocated {c}: {what}" for (f, c) in ((1, 0), (1, 1), (2, 0), (3, 0)) for what in
                  ("the diff = 0 branch", "a = +15, its largest value", "a = -15, its smallest value", "samples below 0 before the clip",
                   "samples above the maximum before the clip")] + ["cclm: k = 1, the smallest shift"])

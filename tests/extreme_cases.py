"""Full-scale worst-case content for the packed 16-bit kernels on the picture chain: content generators and analytic bounds (numpy, int64
throughout), and the pictures built from them.  Used by tests/test_extremes_cpu.py, tests/test_extremes_gpu.py and tools/gen_golden.py;
tests/golden/ref_extremes.json holds the reference's digests.

Content
  plain(kind, ...)     all zero, all maximum, rows / columns / checkerboard of width 1 and 4, the two diagonal stripe patterns of width 2
                       (`diag0` = ((x + y) >> 1) & 1 and `diag1` = ((x - y) >> 1) & 1: full Laplacians along one diagonal, none along the
                       other), and `bands`, which puts the lowest and the highest value of every SAO band side by side.
  sign-matched tiles   per interpolation filter row one 8x8-periodic (luma) / 4x4-periodic (chroma) pattern that holds the sample maximum
                       where sign_h[x] * sign_v[y] > 0 and 0 elsewhere (`tile_mask`), its inverse, and the horizontal-only and
                       vertical-only forms; `pass_bounds` gives the largest and smallest first- and second-pass intermediates by the
                       standard's formulas.

Pictures (none above 136x72, except the CTU-128 ones at 136x136)
  XS0-XS17   SAO: per bit depth six pictures whose (CTB, component) slots walk every band position with the four offsets at
             +-(2^(bd-5) - 1) in four sign patterns, and every edge class with the offsets at both ends, over content that changes per
             16x16 region through all plain patterns.
  XF0-XF10   ALF: 4:2:0 (CTB kernel), 4:4:4 and 4:2:2 (separate chroma / CC-ALF kernels), CTU 32 / 64 / 128, 8 / 10 / 12 bit; the CTBs walk
             the sixteen fixed sets, an APS set whose clip indices are all 0 (clamp-free form) and one with the same coefficient rows and
             clip indices 1 / 2 / 3 (clamped form); the APS rows hold all twelve taps at -128 (centre weight at its most positive), at +127
             (most negative), alternating and drawn from the whole range; chroma alternatives and CC-ALF rows at their range ends.
  XF11-XF14  CC-ALF on luma sign-matched to the CC taps (see CC_TAPS below).
  XR0-XR7, XA0-XA3, XG0-XG3, XI0   regular, affine, GPM and CIIP units on sign-matched tiles (see "inter pictures" below); XA4: affine motion
             that varies per sub-block.

Sensitivity, checked on the CPU with the oracle as stand-in: with the bi-prediction average's sum s0 + s1 computed in int16_t (orc_avg in a
scratch copy of oracle/orc_inter.c) the pictures of SENSITIVE_TO_INT16_SUM no longer hash to their digests, at every bit depth (two 14-bit
intermediates already leave a signed half at 8 bit), while every picture of tests/golden/ref_inter.json still does."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np

import ref_pass_cases as pc
from ffvvc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_extremes.json")
SEED = 0xE87E3000

# ---------------------------------------------------------------------------------------------------------------- plain extremes

PLAIN = ("zero", "max", "rows1", "cols1", "checker1", "rows4", "cols4", "checker4", "diag0", "diag1")


def plain_mask(kind, ys, xs):
    """0 / 1 per sample of the pattern `kind` at the coordinates ys (column vector) and xs (row vector)."""
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    zero = np.zeros(np.broadcast(ys, xs).shape, np.int64)
    if kind == "zero":
        return zero
    if kind == "max":
        return zero + 1
    if kind in ("rows1", "rows4"):
        return zero + ((ys >> (0 if kind == "rows1" else 2)) & 1)
    if kind in ("cols1", "cols4"):
        return zero + ((xs >> (0 if kind == "cols1" else 2)) & 1)
    if kind in ("checker1", "checker4"):
        s = 0 if kind == "checker1" else 2
        return ((ys >> s) + (xs >> s)) & 1
    if kind == "diag0":
        return ((xs + ys) >> 1) & 1
    if kind == "diag1":
        return ((xs - ys) >> 1) & 1
    raise ValueError(kind)


def plain(kind, h, w, bd, y0=0, x0=0):
    """int64 (h, w): the pattern at full scale, 0 and 2^bd - 1; `bands`: the first and the last value of band (x + 3y) % 32 side by side."""
    ys, xs = np.arange(y0, y0 + h)[:, None], np.arange(x0, x0 + w)[None, :]
    if kind == "bands":
        return (((xs + 3 * ys) % 32) << (bd - 5)) + ((xs + ys) & 1) * ((1 << (bd - 5)) - 1)
    return plain_mask(kind, ys, xs) * ((1 << bd) - 1)


def region_planes(dims, bd, kinds, shift, fmt, region=16):
    """Planes whose content changes per region (`region` luma samples a side, scaled to the chroma grid) through `kinds`: region (rx, ry)
    of component c holds kinds[(rx + 3 * ry + shift + c) % len(kinds)]."""
    planes = []
    for c, (pw, ph) in enumerate(dims):
        rw, rh = (region >> fmt[0], region >> fmt[1]) if c else (region, region)
        out = np.zeros((ph, pw), np.int64)
        for ry in range((ph + rh - 1) // rh):
            for rx in range((pw + rw - 1) // rw):
                h, w = min(rh, ph - ry * rh), min(rw, pw - rx * rw)
                out[ry * rh:ry * rh + h, rx * rw:rx * rw + w] = plain(kinds[(rx + 3 * ry + shift + c) % len(kinds)], h, w, bd, ry * rh, rx * rw)
        assert out.min() >= 0 and out.max() < (1 << bd)
        planes.append(out.astype(pc.px(bd)))
    return planes


# ---------------------------------------------------------------------------------------------------------------- SAO pictures

SAO_PER_BD = 6
SAO = [f"XS{i}" for i in range(3 * SAO_PER_BD)]
SAO_KINDS = PLAIN + ("bands",)
SAO_SIGNS = ((1, 1, 1, 1), (-1, -1, -1, -1), (1, -1, 1, -1), (1, 1, -1, -1))          # the last one is what the syntax allows in edge mode
_SAO_FMT = [((1, 1), 3), ((0, 0), 3), ((1, 0), 3), ((1, 1), 3), ((0, 0), 3), ((1, 1), 1)]


def sao_slot(bd_k, rs, c):
    """(type_idx, band position, edge class, signs) of slot (picture k of its bit depth, CTB, component): of nine consecutive slots six are
    band slots and three edge slots; the band slots walk position x sign pattern (the pattern changes from slot to slot, so that every
    picture adds and subtracts), the edge slots class x sign pattern."""
    s = 45 * bd_k + 3 * rs + c
    t = s % 9
    if t < 6:
        b = (s // 9) * 6 + t
        return 1, b % 32, 0, SAO_SIGNS[(b + b // 32) % 4]
    e = (s // 9) * 3 + t - 6
    return 2, 0, e % 4, SAO_SIGNS[(e // 4) % 4]


def _sao_picture(i):
    bd, k = (8, 10, 12)[i // SAO_PER_BD], i % SAO_PER_BD
    fmt, n_comp = _SAO_FMT[k]
    rng = np.random.default_rng(SEED + i)
    lf = (k & 1, (k >> 1) & 1)
    fp = pc.draw_filter(f"XS{i}", rng, bd, fmt, n_comp, 5, (136, 72), 1 + k % 3, bool(k & 1), lf, planes=False)
    t = fp.t
    assert t.cw * t.ch == 15
    fp.planes = region_planes(fp.dims, bd, SAO_KINDS, 2 * i, fmt)
    tab = (abi.SaoCtb * (t.cw * t.ch))()
    top = (1 << (bd - 5)) - 1
    for rs in range(t.cw * t.ch):
        for c in range(3):
            ty, pos, eo, signs = sao_slot(k, rs, c if n_comp == 3 else (c + rs) % 3)          # luma alone walks all three slot kinds
            tab[rs].type_idx[c], tab[rs].band_position[c], tab[rs].eo_class[c] = ty, pos, eo
            for q in range(4):
                tab[rs].offset_val[c][q + 1] = signs[q] * top
    fp.sao = np.frombuffer(bytes(tab), np.uint8).copy()
    fp.stages = ("sao",)
    return fp


# ---------------------------------------------------------------------------------------------------------------- ALF pictures

# bit depth, (hs, vs), CTU log2, size
_ALF = [
    dict(bd=12, fmt=(1, 1), ctb_log2=5, size=(136, 72)),
    dict(bd=10, fmt=(1, 1), ctb_log2=6, size=(136, 72)),
    dict(bd=8, fmt=(1, 1), ctb_log2=7, size=(136, 136)),
    dict(bd=12, fmt=(1, 1), ctb_log2=7, size=(136, 136)),
    dict(bd=10, fmt=(0, 0), ctb_log2=5, size=(136, 72)),
    dict(bd=12, fmt=(0, 0), ctb_log2=6, size=(136, 72)),
    dict(bd=8, fmt=(1, 0), ctb_log2=5, size=(136, 72)),
    dict(bd=12, fmt=(1, 0), ctb_log2=6, size=(136, 72)),
    dict(bd=8, fmt=(1, 1), ctb_log2=5, size=(136, 72)),
    dict(bd=12, fmt=(1, 1), ctb_log2=6, size=(136, 72)),
    dict(bd=10, fmt=(1, 1), ctb_log2=5, size=(136, 72)),
]
ALF = [f"XF{i}" for i in range(len(_ALF))]
ALF_COEFF_MIN, ALF_COEFF_MAX = -128, 127       # alf_luma_coeff / alf_chroma_coeff per tap, the ends the pictures use of the standard's range per tap
CC_COEFF_MAX = 64                              # alf_cc_*_mapped_coeff_abs: 0 or 2^(k - 1), k <= 7


ALF_REACHED = (0, 4, 9, 14, 19, 24)            # classes that full-scale content reaches: the activity is 0 or saturates at 4 (asserted by the test)


def alf_rows(rng, n, taps):
    """Coefficient rows at the range ends: all at the minimum, all at the maximum, alternating both ways; the other rows are drawn from
    the whole range.  Of a luma set's 25 rows the six that full-scale content reaches (ALF_REACHED) take the four extreme forms."""
    alt = np.where(np.arange(taps) & 1, ALF_COEFF_MIN, ALF_COEFF_MAX)
    forms = [np.full(taps, ALF_COEFF_MIN), np.full(taps, ALF_COEFF_MAX), alt, -1 - alt]
    which = {0: 0, 4: 1, 9: 2, 14: 3, 19: 1, 24: 0} if n == 25 else {r: r % 4 for r in range(n)}
    rows = np.array([forms[which[r]] if r in which else rng.integers(ALF_COEFF_MIN, ALF_COEFF_MAX + 1, size=taps) for r in range(n)], np.int64)
    assert rows.min() >= ALF_COEFF_MIN and rows.max() <= ALF_COEFF_MAX
    return rows.astype(np.int16)


def alf_set_of(i, rs):
    """filt_set_idx_y of CTB rs of picture i: APS set 16 (clip indices 0), APS set 17 (clip indices 1..3), then the fixed sets in turn."""
    q = rs + i
    return (16, 17, (q // 3 + 5 * i) % 16)[q % 3]


def _alf_picture(i):
    c = _ALF[i]
    bd, fmt = c["bd"], c["fmt"]
    rng = np.random.default_rng(SEED + 100 + i)
    fp = pc.draw_filter(f"XF{i}", rng, bd, fmt, 3, c["ctb_log2"], c["size"], 1, False, (1, 1), planes=False)
    t = fp.t
    fp.shift = 3 * i
    fp.planes = region_planes(fp.dims, bd, PLAIN, fp.shift, fmt)
    n_ctb = t.cw * t.ch
    tab = (abi.AlfCtb * n_ctb)()
    for rs in range(n_ctb):
        for comp in range(3):
            tab[rs].ctb_flag[comp] = 1
        tab[rs].filt_set_idx_y = alf_set_of(i, rs)
        for comp in range(2):
            tab[rs].alt_idx[comp], tab[rs].cc_idc[comp] = (rs + 3 * comp + i) % 8, (rs + 2 * comp + i) % 5
    fp.alf = np.frombuffer(bytes(tab), np.uint8).copy()
    luma = alf_rows(rng, 25, 12)
    chroma = alf_rows(rng, 4, 6)
    cc = np.array([[CC_COEFF_MAX] * 7, [-CC_COEFF_MAX] * 7, [CC_COEFF_MAX, -CC_COEFF_MAX] * 3 + [CC_COEFF_MAX],
                   [-CC_COEFF_MAX, CC_COEFF_MAX] * 3 + [-CC_COEFF_MAX]], np.int16)
    # both luma sets carry the same rows (slice 1 would list them in the other order; these pictures have one slice); set 0: clip indices 0,
    # set 1: 1 / 2 / 3 mixed.  Chroma alternatives 0-3: clip indices 0, 4-7: the same rows with 1 / 2 / 3.
    fp.aps = [luma, luma.copy(), np.zeros((25, 12), np.uint8), rng.integers(1, 4, size=(25, 12)).astype(np.uint8),
              np.concatenate([chroma, chroma]), np.concatenate([np.zeros((4, 6), np.uint8), rng.integers(1, 4, size=(4, 6)).astype(np.uint8)]),
              cc, cc[::-1].copy()]
    assert fp.n_slices == 1 and int(fp.alf.reshape(n_ctb, 8)[:, 3].max()) < 18
    fp.stages = ("alf",)
    return fp


# ---- CC-ALF on luma sign-matched to the CC taps: XF11-XF14.  A chroma sample reads the co-located luma sample c and its neighbours l_k at
# CC_TAPS, sum = sum_k g[k] * (l_k - c) (vvc_filter_template.c: alf_filter_cc).  Over content in 0 .. top the sum lies in
# +-top * max(P, N), P / N = the sum of the positive / negative coefficients' magnitudes.  A 4x4-periodic luma tile holds the maximum under
# the taps of one sign and 0 under the centre and everything else; with its inverse (centre at the maximum) the chroma samples whose
# co-located luma sample sits on the 4-grid reach both ends.  Every 16x16 luma region is matched to the CTB's Cb row (even region columns) or
# Cr row (odd), tile in even region rows, inverse in odd.  Cb is flat at mid-range, so that an unsaturated correction is seen as it is; Cr
# holds the plain patterns, so that the sample clip bites too.  Rows 2 of Cb and 2, 3 of Cr stay below the correction's clip 2^(bd - 1).

CC_TAPS = ((0, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1), (0, 2))          # (dx, dy) of filter[0..6]
CC_ROWS = (np.array([[64] * 7, [64, -64, 64, -64, 64, -64, 64], [1, -2, 4, -8, 16, -32, 2], [-64, -32, -16, -8, -4, -2, -1]], np.int16),
           np.array([[-64] * 7, [-64, 64, -64, 64, -64, 64, -64], [-1, 2, -4, 8, -16, 32, -2], [8] * 7], np.int16))
_ALF_CC = [
    dict(bd=12, fmt=(1, 1), ctb_log2=5, size=(136, 72)),
    dict(bd=12, fmt=(0, 0), ctb_log2=5, size=(136, 72)),
    dict(bd=10, fmt=(1, 0), ctb_log2=6, size=(136, 72)),
    dict(bd=8, fmt=(1, 1), ctb_log2=6, size=(136, 72)),
]
ALF_CC = [f"XF{len(_ALF) + i}" for i in range(len(_ALF_CC))]


def cc_bound(g):
    """max(P, N) of a CC row: the sum's extremes are +- top times this."""
    g = np.asarray(g, np.int64)
    return int(max(np.where(g > 0, g, 0).sum(), -np.where(g < 0, g, 0).sum()))


def cc_tile(g, inverse=False):
    """0 / 1 (4, 4), index [y % 4][x % 4] around a centre on the 4-grid: 1 under the taps of the heavier sign, 0 under the centre and
    elsewhere; `inverse` swaps 0 and 1."""
    g = np.asarray(g, np.int64)
    heavy = 1 if np.where(g > 0, g, 0).sum() >= -np.where(g < 0, g, 0).sum() else -1
    m = np.zeros((4, 4), np.int64)
    for k, (dx, dy) in enumerate(CC_TAPS):
        if g[k] * heavy > 0:
            m[dy % 4, dx % 4] = 1
    assert m[0, 0] == 0
    return 1 - m if inverse else m


def cc_region(t, alf, rx, ry):
    """(component 1 / 2 the 16x16 luma region is matched to, its CC row or None when CC-ALF is off for it in the region's CTB, inverse)."""
    rs = ((16 * ry) >> t.ctb_log2) * t.cw + ((16 * rx) >> t.ctb_log2)
    comp = 1 + (rx & 1)
    idc = int(alf.reshape(-1, 8)[rs, 5 + comp])
    return comp, (CC_ROWS[comp - 1][idc - 1] if idc else None), bool(ry & 1)


def _alf_cc_picture(i):
    c = _ALF_CC[i]
    bd, fmt = c["bd"], c["fmt"]
    name = ALF_CC[i]
    rng = np.random.default_rng(SEED + 150 + i)
    fp = pc.draw_filter(name, rng, bd, fmt, 3, c["ctb_log2"], c["size"], 1, False, (1, 1), planes=False)
    t = fp.t
    n_ctb = t.cw * t.ch
    tab = (abi.AlfCtb * n_ctb)()
    for rs in range(n_ctb):
        tab[rs].ctb_flag[0] = 1
        tab[rs].ctb_flag[1] = tab[rs].ctb_flag[2] = rs & 1          # chroma ALF under the correction in every other CTB
        tab[rs].filt_set_idx_y = alf_set_of(i, rs)
        tab[rs].alt_idx[0], tab[rs].alt_idx[1] = rs % 8, (rs + 3) % 8
        tab[rs].cc_idc[0], tab[rs].cc_idc[1] = 1 + (rs + 2) % 4, (rs + rs // 5 + 3) % 5          # the first CTB takes the unsaturated rows
    fp.alf = np.frombuffer(bytes(tab), np.uint8).copy()
    top = (1 << bd) - 1
    luma = plain("checker4", t.height, t.width, bd)
    for ry in range((t.height + 15) // 16):
        for rx in range((t.width + 15) // 16):
            _comp, g, inv = cc_region(t, fp.alf, rx, ry)
            if g is None:
                continue
            h, w = min(16, t.height - 16 * ry), min(16, t.width - 16 * rx)
            ys, xs = np.arange(16 * ry, 16 * ry + h)[:, None], np.arange(16 * rx, 16 * rx + w)[None, :]
            luma[16 * ry:16 * ry + h, 16 * rx:16 * rx + w] = cc_tile(g, inv)[ys % 4, xs % 4] * top
    (cw, chh) = fp.dims[1]
    fp.planes = [luma.astype(pc.px(bd)), np.full((chh, cw), 1 << (bd - 1), pc.px(bd)), region_planes(fp.dims, bd, PLAIN, i, fmt)[2]]
    fp.aps = [alf_rows(rng, 25, 12), alf_rows(rng, 25, 12), np.zeros((25, 12), np.uint8), rng.integers(1, 4, size=(25, 12)).astype(np.uint8),
              np.concatenate([alf_rows(rng, 4, 6)] * 2), np.concatenate([np.zeros((4, 6), np.uint8), rng.integers(1, 4, size=(4, 6)).astype(np.uint8)]),
              CC_ROWS[0].copy(), CC_ROWS[1].copy()]
    assert fp.n_slices == 1
    fp.stages = ("alf",)
    return fp


_filter = {}


def filter_picture(name):
    """XS* / XF*, made once per process; nobody writes to a picture."""
    if name not in _filter:
        i = int(name[2:])
        _filter[name] = _sao_picture(i) if name in SAO else _alf_picture(i) if name in ALF else _alf_cc_picture(i - len(_ALF))
    return _filter[name]


def filter_digests(name, run_f):
    """The record of ref_extremes.json for an SAO / ALF picture, from run_f(fp, stage): the inputs and one digest per output plane."""
    fp = filter_picture(name)
    rec = {"inputs": pc.filter_inputs_digest(fp)}
    rec.update(pc.stage_digests({s: run_f(fp, s) for s in fp.stages}, fp.stages))
    return rec


# ---------------------------------------------------------------------------------------------------------------- ALF by its own rules

def alf_classify(luma, bd, ctb_log2):
    """Per 4x4 block of the picture: sums (nby, nbx, 4) = V, H, D0, D1 over the block's window, rowmax = the largest sum of one cell row of
    the window (four cells side by side) per direction, class and transpose index, by vvc_filter_template.c's alf_classify / alf_get_idx
    with the virtual boundary of every CTB at ctb - 4; `inner` marks the blocks whose window stays inside the picture (the others see the
    picture extended by its own border samples here, which nothing relies on).

    A cell starts at an even (Y, X) and adds the Laplacians of sample A = (Y, X) and sample B = (Y + 1, X + 1) (:326-341, with src moved up
    three rows and left two); a block at (y, x) sums the cells at Y = y - 2, y, y + 2, y + 4 and X = x - 2 .. x + 4 (:357-373).  At the
    boundary the sample row vb - 1 takes its own row for the row below and the sample row vb its own row for the row above (:321-324);
    the block row that ends at the boundary drops its last cell row, the one that starts there its first, and both scale by 3 (:350-356)."""
    H, W = luma.shape
    ctb, vb = 1 << ctb_log2, (1 << ctb_log2) - 4
    p = np.pad(luma.astype(np.int64), 4, mode="edge")
    Hp, Wp = H + 6, W + 6                                                   # index (j, i) = picture sample (j - 3, i - 3)
    at = lambda dy, dx: p[1 + dy:1 + dy + Hp, 1 + dx:1 + dx + Wp]          # noqa: E731
    yc = (np.arange(-3, H + 3) % ctb)[:, None]
    up = lambda dx: np.where(yc == vb, at(0, dx), at(-1, dx))              # noqa: E731
    dn = lambda dx: np.where(yc == vb - 1, at(0, dx), at(1, dx))           # noqa: E731
    c2 = 2 * at(0, 0)
    lap = np.stack([np.abs(c2 - up(0) - dn(0)), np.abs(c2 - at(0, -1) - at(0, 1)), np.abs(c2 - up(-1) - dn(1)), np.abs(c2 - up(1) - dn(-1))])
    K, L = H // 2 + 2, W // 2 + 2                                           # cell (k, l) starts at picture (2k - 2, 2l - 2)
    cell = lap[:, 1::2, 1::2][:, :K, :L] + lap[:, 2::2, 2::2][:, :K, :L]
    nby, nbx = H // 4, W // 4
    rsum = sum(cell[:, :, j:j + 2 * nbx:2] for j in range(4))               # [dir][cell row][block column]
    rows = np.stack([rsum[:, i:i + 2 * nby:2] for i in range(4)], 1)        # [dir][i][block row][block column]
    yr = (4 * np.arange(nby) % ctb)[None, None, :, None]
    on = np.ones((1, 4, nby, 1), bool)
    on[:, 3] &= yr[:, 0] + 4 != vb
    on[:, 0] &= yr[:, 0] != vb
    ac = np.where((yr[0, 0] + 4 == vb) | (yr[0, 0] == vb), 3, 2)           # (nby, 1)
    rows = np.where(on, rows, 0)
    s = rows.sum(1)                                                         # [dir][block row][block column]
    rowmax = rows.max(1)
    v, h, d0, d1 = s
    dir_hv, hv1, hv0 = (v <= h).astype(np.int64), np.maximum(v, h), np.minimum(v, h)
    dir_d, dd1, dd0 = (d0 <= d1).astype(np.int64), np.maximum(d0, d1), np.minimum(d0, d1)
    dir1 = (dd1 * hv0 <= hv1 * dd0).astype(np.int64)
    hvd1, hvd0 = np.where(dir1, hv1, dd1), np.where(dir1, hv0, dd0)
    arg_var = np.array([0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4])
    cls = arg_var[np.clip(((v + h) * ac) >> (bd - 1), 0, 15)]
    cls = cls + np.where(hvd1 * 2 > 9 * hvd0, ((dir1 << 1) + 2) * 5, np.where(hvd1 > 2 * hvd0, ((dir1 << 1) + 1) * 5, 0))
    by, bx = np.arange(nby)[:, None], np.arange(nbx)[None, :]
    inner = (by > 0) & (by < nby - 1) & (bx > 0) & (bx < nbx - 1)
    return SimpleNamespace(sums=np.moveaxis(s, 0, -1), rowmax=np.moveaxis(rowmax, 0, -1), cls=cls, tr=dir_d * 2 + dir_hv, inner=inner)


# ---------------------------------------------------------------------------------------------------------------- sign-matched tiles

_tables = {}


def filter_rows():
    """(luma int64 [3][16][8], chroma int64 [3][32][4]): ff_vvc_inter_luma_filters (regular, half-pel alternative, affine 6-tap) and
    ff_vvc_inter_chroma_filters as the built library exports them (tests/test_tables_cpu.py holds them to the reference's files)."""
    if not _tables:
        lib = ctypes.CDLL(abi.LIB_PATH)
        _tables["luma"] = np.array((ctypes.c_int8 * 384).in_dll(lib, "vvc355_tab_inter_luma_filters"), np.int64).reshape(3, 16, 8)
        _tables["chroma"] = np.array((ctypes.c_int8 * 384).in_dll(lib, "vvc355_tab_inter_chroma_filters"), np.int64).reshape(3, 32, 4)
    return _tables["luma"], _tables["chroma"]


def luma_phases():
    """(0, 8, a, b): the integer position, the half-sample position and the two other phases whose regular filter row has the largest
    positive tap sum."""
    luma, _ = filter_rows()
    pos = np.where(luma[0] > 0, luma[0], 0).sum(1)
    rest = sorted((p for p in range(1, 16) if p != 8), key=lambda p: (-int(pos[p]), p))
    return (0, 8, rest[0], rest[1])


def tap_signs(row):
    """Sign of the tap that reads column / row i of the periodic tile (period = number of taps), for an output sample on the period's grid:
    tap k reads position k - lead, lead = 3 (8 taps) or 1 (4 taps)."""
    n = len(row)
    lead = 3 if n == 8 else 1
    out = np.zeros(n, np.int64)
    for k in range(n):
        out[(k - lead) % n] = np.sign(row[k])
    return out


def tile_mask(hrow, vrow, form="hv", inverse=False):
    """0 / 1 (n, n), n = taps: 1 where sign_h[x] * sign_v[y] > 0 ("hv"), where sign_h[x] > 0 ("h": horizontal-only) or where sign_v[y] > 0
    ("v"); `inverse` swaps 0 and 1."""
    sh, sv = tap_signs(hrow)[None, :], tap_signs(vrow)[:, None]
    m = sh * sv > 0 if form == "hv" else sh + 0 * sv > 0 if form == "h" else sv + 0 * sh > 0
    m = m.astype(np.int64)
    return 1 - m if inverse else m


def pass_bounds(hrow, vrow, fx, fy, bd):
    """By the standard's formulas (8.5.6.3: shift1 = bd - 8 after the first pass, shift2 = 6 after the second, shift3 = 14 - bd at the
    integer position), in int64: {"first": (smallest, largest) intermediate after the first pass, "second": after the second} over all
    content in 0 .. 2^bd - 1.  With one fractional component the one pass is both; with none the sample is scaled to 14 bits."""
    top = np.int64((1 << bd) - 1)
    pos = lambda r: np.int64(np.where(r > 0, r, 0).sum())          # noqa: E731
    neg = lambda r: np.int64(np.where(r < 0, r, 0).sum())          # noqa: E731
    if not fx and not fy:
        b = (np.int64(0), top << (14 - bd))
        return {"first": b, "second": b}
    one = hrow if fx else vrow
    first = ((neg(one) * top) >> (bd - 8), (pos(one) * top) >> (bd - 8))
    if not (fx and fy):
        return {"first": first, "second": first}
    second = ((pos(vrow) * first[0] + neg(vrow) * first[1]) >> 6, (pos(vrow) * first[1] + neg(vrow) * first[0]) >> 6)
    return {"first": first, "second": second}


def intermediate(plane, x, y, hrow, vrow, fx, fy, bd):
    """The 14-bit-scaled intermediate of the sample whose window starts at integer position (x, y) of `plane`, in int64, by the same
    formulas: (values after the first pass that the sample reads, value after the last pass)."""
    p = plane.astype(np.int64)
    n = len(hrow)
    lead = 3 if n == 8 else 1
    if not fx and not fy:
        v = p[y, x] << (14 - bd)
        return np.array([v]), v
    if fx and fy:
        first = np.array([(hrow * p[y - lead + r, x - lead:x - lead + n]).sum() >> (bd - 8) for r in range(n)])
        return first, (vrow * first).sum() >> 6
    v = ((hrow * p[y, x - lead:x - lead + n]).sum() if fx else (vrow * p[y - lead:y - lead + n, x]).sum()) >> (bd - 8)
    return np.array([v]), v


def chroma_phase(f, shift):
    """The chroma filter phase (1/32) of the luma motion fraction f (1/16) for a component subsampled by `shift` (vvc_inter.c: the motion is
    read in 1/32 of a chroma sample where the component is subsampled, doubled where it is not)."""
    return (f & ((1 << (4 + shift)) - 1)) << (1 - shift)


# ---------------------------------------------------------------------------------------------------------------- inter pictures
#
# Every unit is 16x16 (XR7: one 128x128 unit) at a multiple of 16 with motion below one sample, so the output samples at multiples of 8 that
# lie at least 3 inside the unit ("marked": (x0 + 8, y0 + 8) in a 16x16 unit) read nothing but the unit's own tile.  Reference picture 0 of
# either list holds the sign-matched tile of the unit's phase pair for that list, reference picture 1 its inverse: ref_idx picks the end.
# Four slices: 0 default weights + LMCS, 1 B-typed explicit weights, 2 P-typed explicit weights + LMCS, 3 default weights, no LMCS.
# Explicit weights sit at the ends of what pred_weight_table() can code with the pictures' denominators (2^denom - 128 .. 2^denom + 127,
# offsets -128 .. 127): list 0: ref_idx 0 largest weight and offset, 1 smallest; list 1: ref_idx 0 smallest weight with the largest offset,
# 1 the reverse; odd pictures swap the two lists' tables.

import ref_inter_cases as ic          # noqa: E402
import inter_frame_cases as ifc       # noqa: E402

# name -> bit depth, chroma_format_idc
_REGULAR = [dict(bd=8, idc=1), dict(bd=10, idc=1), dict(bd=12, idc=1), dict(bd=8, idc=3), dict(bd=10, idc=3), dict(bd=12, idc=3), dict(bd=12, idc=2),
            dict(bd=12, idc=1, big=True)]
REGULAR = [f"XR{i}" for i in range(len(_REGULAR))]
# XA4: motion that varies from sub-block to sub-block (a four-parameter field in even units, a six-parameter one in odd units), on plain
# full-scale patterns: every 4x4 sub-block of a unit has its own phase pair, which the tile pictures cannot give
_AFFINE = [dict(bd=8, idc=1), dict(bd=10, idc=3), dict(bd=12, idc=1), dict(bd=12, idc=2), dict(bd=12, idc=1, varying=True)]
VARYING = ("XA4",)
AFFINE = [f"XA{i}" for i in range(len(_AFFINE))]
_GPM = [dict(bd=8, idc=1), dict(bd=10, idc=2), dict(bd=12, idc=1), dict(bd=12, idc=3)]
GPM = [f"XG{i}" for i in range(len(_GPM))]
CTU_SLICE = [0, 1, 2, 3, 0, 3, 2, 1, 0, 0, 0, 0, 0, 0, 0]          # 5 x 3 CTUs of 32: every slice holds eight 16x16 units
DMV_BOUND = 31                                                     # PROF's motion differences are clipped to -31 .. 31 (vvc_mvs.c: dmv_limit)
SENSITIVE_TO_INT16_SUM = ("XR0", "XR1", "XR2", "XR3", "XR4", "XR5", "XR6", "XR7", "XA0", "XA1", "XA2", "XA3", "XI0")


def extreme_slices(flip):
    slices = (abi.InterSlice * 4)()
    slices[0].lmcs_used = 1
    slices[1].weighted_bipred = 1
    slices[2].weighted_pred, slices[2].lmcs_used = 1, 1
    for s in (slices[1], slices[2]):
        s.log2_denom[0], s.log2_denom[1] = 6, 5
        for l in range(2):
            for c in range(3):
                one = 1 << s.log2_denom[c > 0]
                ends = [(one + 127, 127), (one - 128, -128)] if (l ^ flip) == 0 else [(one - 128, 127), (one + 127, -128)]
                for r in range(2):
                    s.weight[l][c][r], s.offset[l][c][r] = ends[r]
    return slices


class _Units:
    """Places units by hand on a ref_inter_cases.Picture and remembers what each one reads: the hooks of one picture."""

    def __init__(self, i, kind, big=False, varying=False):
        self.i, self.kind, self.big, self.varying, self.m = i, kind, big, varying, 3 * i
        self.read = []          # per unit: dict(x, y, w, h, kind, lists={l: (fx, fy, ref_idx, content)}, hpel, dmvr, bdof, bcw, slice, prof)

    def phases(self):
        """The next (fx, fy, inverse) of the walk over every phase pair on the tile and on its inverse."""
        ph = luma_phases()
        m, self.m = self.m, self.m + 1
        return ph[m % 4], ph[(m // 4) % 4], (m // 16) % 2

    def layout(self, pic):
        pic.slices = extreme_slices(self.i & 1)
        pus, aff, gpm = [], [], []
        if self.big:
            pic.ctu_slice = [3] * (pic.ncx * pic.ncy)          # default weights, no LMCS
            cells = [(0, 0, 128, 128, 3)]
        else:
            assert pic.ncx * pic.ncy == len(CTU_SLICE)
            pic.ctu_slice = list(CTU_SLICE)
            cells = [(x, y, 16, 16, CTU_SLICE[(y // 32) * pic.ncx + x // 32]) for y in range(0, 64, 16) for x in range(0, 128, 16)]
        per_slice = {}
        for (x, y, w, h, sl) in cells:
            j = per_slice.get(sl, 0)
            per_slice[sl] = j + 1
            u = dict(x=x, y=y, w=w, h=h, kind=self.kind, slice=sl, hpel=0, dmvr=0, bdof=0, bcw=0, prof=0, lists={})
            explicit = sl in (1, 2)
            if self.kind == "R":
                if self.big:
                    pf = 3
                elif sl == 2:
                    pf = 1                                     # a P slice predicts from list 0
                else:
                    pf = (1, 2, 3, 3, 3, 3, 3, 3)[j]
                if not self.big and not explicit:
                    u["bcw"] = (0, 0, 0, 1 + (self.i + j + (sl == 3)) % 4, 1 + (self.i + j + 2 + (sl == 3)) % 4, 0, 0, 0)[j]
                    u["dmvr"], u["bdof"] = (0, 0, 0, 0, 0, 1, 0, 1)[j], (0, 0, 0, 0, 0, 0, 1, 1)[j]
            elif self.kind == "A":
                pf = 1 if sl == 2 else (1, 2, 3, 3, 3, 3, 1, 3)[j]
                u["bcw"] = (1 + (self.i + j) % 4) if (not explicit and pf == 3 and j in (3, 5)) else 0
                u["prof"] = (0, 0, 0, 0, 3, 3, 1, 1)[j]
            else:
                pf = 3                                          # both lists hold one part each
            search = u["dmvr"] or u["bdof"]
            plain_pairs = (("zero", "max"), ("checker1", "checker1i"), None)
            for l in range(2):
                if not pf & (1 << l):
                    continue
                fx, fy, inv = self.phases()
                content = ("tile", "hv")
                if search:
                    pair = plain_pairs[(self.i + (sl == 3) + (j - 5)) % 3]
                    content = ("plain", pair[l]) if pair else ("tile", ("h", "v")[l])
                if self.varying:
                    content = ("plain", ("checker1", "rows1", "cols1", "diag0", "diag1", "checker4")[(len(self.read) + 3 * l) % 6])
                if self.kind == "G" and l == 1:                 # the other part: the same phase pair on the inverse
                    fx, fy, inv = u["lists"][0][0], u["lists"][0][1], 1 - u["lists"][0][2]
                u["lists"][l] = (fx, fy, inv, content)
            if self.kind == "R" and not search and all(f in (0, 8) for v in u["lists"].values() for f in v[:2]) and any(v[0] == 8 or v[1] == 8 for v in u["lists"].values()):
                u["hpel"] = (x // 16 + y // 16) & 1            # every fraction 0 or 1/2 and at least one 1/2: the alternative filter for every other such unit
            blk = pic.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
            blk["ref_idx"] = [u["lists"][0][2] if pf & 1 else -1, u["lists"][1][2] if pf & 2 else -1]
            for l, v in u["lists"].items():
                blk["mv"][:, :, l, 0], blk["mv"][:, :, l, 1] = v[0], v[1]
            blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"] = u["hpel"], u["bcw"], pf
            if self.varying:
                k = len(self.read)
                sy_, sx_ = np.mgrid[0:h // 4, 0:w // 4]
                for l in u["lists"]:
                    a, b, c_, d = 5 + 3 * k + l, 11 - 2 * k, 7 + k, -9 + 4 * l + k          # per sub-block, 1/16 sample
                    if k % 2 == 0:
                        c_, d = -b, a                              # four parameters: rotation and zoom
                    blk["mv"][:, :, l, 0] += (-1) ** k * 16 * (k % 3) + a * sx_ + c_ * sy_
                    blk["mv"][:, :, l, 1] += (-1) ** l * 16 * (k % 2) + b * sx_ + d * sy_
            pic.covered[y:y + h, x:x + w] = True
            pic.units.append((self.kind, x, y, w, h))
            if self.kind == "R":
                ns = (max(1, w // 16), max(1, h // 16)) if search else (1, 1)
                pus.append((x, y, w, h, ns[0], ns[1], u["dmvr"], u["bdof"], 0, u["hpel"], sl, 0, 0))
            elif self.kind == "A":
                # PROF's motion differences at both clip bounds, the sign changing from sample to sample and from list to list
                dmv = np.zeros((2, 2, 16), np.int64)
                k = np.arange(16)
                for l in range(2):
                    dmv[l, 0], dmv[l, 1] = np.where((k + l) & 1, -DMV_BOUND, DMV_BOUND), np.where(((k >> 2) + l) & 1, DMV_BOUND, -DMV_BOUND)
                aff.append((x, y, w, h, u["prof"], sl, dmv))
            else:
                mvs = []
                for l in range(2):
                    m = np.zeros((), ifc.MVF_DT)
                    m["pred_flag"], m["ref_idx"] = l + 1, [-1, -1]
                    m["ref_idx"][l] = u["lists"][l][2]
                    m["mv"][l] = u["lists"][l][:2]
                    mvs.append(m)
                u["partition"] = (16 * self.i + len(gpm)) % 64
                gpm.append((x, y, w, h, u["partition"], sl, mvs))
            self.read.append(u)
        return pus, aff, gpm

    def rows(self, u, l, c):
        """(horizontal row, vertical row, fx, fy) of the filter that list l of unit u reads component c with."""
        luma, chroma = filter_rows()
        fx, fy = u["lists"][l][:2]
        if c == 0:
            t = 2 if self.kind == "A" else u["hpel"]
            return luma[t][fx], luma[t][fy], fx, fy
        return chroma[0][chroma_phase(fx, self.pic.hs)], chroma[0][chroma_phase(fy, self.pic.vs)], chroma_phase(fx, self.pic.hs), chroma_phase(fy, self.pic.vs)

    def content(self, pic):
        """refs[list][ref_idx][component]: checker4 where no unit reads; per unit and list the tile of its phase pair in reference picture 0 and
        the inverse tile in reference picture 1 (or the plain pattern, in both)."""
        self.pic = pic
        top = (1 << pic.bd) - 1
        refs = [[[plain("checker4", ph, pw, pic.bd) for (pw, ph) in pic.dims] for r in range(2)] for l in range(2)]
        for u in self.read:
            for l, (fx, fy, inv, content) in u["lists"].items():
                for c in range(3 if pic.chroma else 1):
                    hs, vs = (pic.hs, pic.vs) if c else (0, 0)
                    x, y, w, h = u["x"] >> hs, u["y"] >> vs, u["w"] >> hs, u["h"] >> vs
                    ys, xs = np.arange(y, y + h)[:, None], np.arange(x, x + w)[None, :]
                    for r in range(2):
                        if content[0] == "plain":
                            kind = content[1]
                            m = 1 - plain_mask(kind[:-1], ys, xs) if kind.endswith("i") else plain_mask(kind, ys, xs)
                        else:
                            hrow, vrow, _, _ = self.rows(u, l, c)
                            t = tile_mask(hrow, vrow, content[1], inverse=bool(r))
                            m = t[ys % t.shape[0], xs % t.shape[1]]
                        refs[l][r][c][y:y + h, x:x + w] = m * top
        return [[[a.astype(ic.px(pic.bd)) for a in r] + ([] if pic.chroma else [np.zeros((pic.height, pic.width), ic.px(pic.bd))] * 2)
                 for r in l] for l in refs]


_inter = {}


def inter_picture(name):
    """XR* / XA* / XG*, made once per process: (picture, the _Units that placed it)."""
    if name not in _inter:
        kind, i = name[1], int(name[2:])
        c = {"R": _REGULAR, "A": _AFFINE, "G": _GPM}[kind][i]
        u = _Units(i + {"R": 0, "A": 20, "G": 40}[kind], kind, big=c.get("big", False), varying=c.get("varying", False))
        big = c.get("big", False)
        pic = ic.Picture(name, np.random.default_rng(SEED + 200 + sum(map(ord, name))), c["bd"], c["idc"], 7 if big else 5, (136, 136) if big else (136, 72),
                         kind, content=u.content, layout=u.layout)
        _inter[name] = (pic, u)
    return _inter[name]


# ---- CIIP: XI0, 12 bit 4:2:0.  16x16 units on the black squares of the 16-grid's checkerboard, so that the blocks above and to the left are
# background (intra or inter at random: intra weights 1, 2 and 3); the inter half on sign-matched tiles as in the regular pictures.

import ciip_frame_cases as cc          # noqa: E402

CIIP = ["XI0"]
_ciip = {}


def ciip_picture(name="XI0"):
    """(picture in the form of ref_inter_cases.ciip_picture, the _Units that hold what every unit reads)."""
    if name not in _ciip:
        bd, idc, W, H = 12, 1, 136, 72
        rng = np.random.default_rng(SEED + 300)
        p = cc.CiipPicture(W, H, 5, idc, 2)
        p.bd, p.mv_range = bd, 16
        p.slice_idx[:] = (np.arange(p.ncx * p.ncy) // p.ncx > 0).astype(np.int16)
        p.slices = cc.make_slices(rng)
        ext = extreme_slices(0)[1]
        for l in range(2):
            for c in range(3):
                for r in range(16):
                    p.slices[1].weight[l][c][r], p.slices[1].offset[l][c][r] = ext.weight[l][c][r], ext.offset[l][c][r]
        cc.fill_background(rng, p.mvf)
        u = _Units(60, "R")
        units = []
        for y in range(0, 64, 16):
            for x in range(0, 128, 16):
                if (x // 16 + y // 16) & 1:
                    continue
                j = len(units)
                pf = (1, 2, 3, 3)[j % 4]
                sl = int(p.slice_idx[(y >> 5) * p.ncx + (x >> 5)])
                rec = dict(x=x, y=y, w=16, h=16, kind="R", slice=sl, hpel=0, dmvr=0, bdof=0, bcw=(1 + j % 4) if (pf == 3 and j % 8 == 3) else 0, prof=0, lists={})
                for l in range(2):
                    if pf & (1 << l):
                        fx, fy, inv = u.phases()
                        rec["lists"][l] = (fx, fy, inv, ("tile", "hv"))
                blk = p.mvf[y // 4:(y + 16) // 4, x // 4:(x + 16) // 4]
                blk["ref_idx"] = [rec["lists"][0][2] if pf & 1 else -1, rec["lists"][1][2] if pf & 2 else -1]
                blk["mv"] = 0
                for l, v in rec["lists"].items():
                    blk["mv"][:, :, l, 0], blk["mv"][:, :, l, 1] = v[0], v[1]
                blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"], blk["ciip_flag"] = 0, rec["bcw"], pf, 1
                units.append((x, y, 16, 16, 0, sl))
                u.read.append(rec)
        p.set_records(rng, units)
        cc.build_commands(rng, p)
        dims = [(W, H)] + [(W >> p.hs, H >> p.vs)] * 2
        refs = u.content(SimpleNamespace(bd=bd, dims=dims, hs=p.hs, vs=p.vs, chroma=True, width=W, height=H))
        lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(np.uint16)
        _ciip[name] = (SimpleNamespace(name=name, p=p, bd=bd, dims=dims, refs=refs, lut=lut, sentinel=(1 << bd) // 3, n_comp=3), u)
    return _ciip[name]


def ciip_digests(name, run_i):
    cp, _ = ciip_picture(name)
    out = run_i(cp)
    rec = {"inputs": ic.ciip_inputs_digest(cp), **ic.plane_digests(out.planes)}
    rec.update(scratch=ic.sha(out.scratch), weights=ic.sha(out.weights), joint=ic.sha(ic.ciip_joint(cp, out.weights)))
    return rec


def marked(u):
    """Luma positions of unit u whose window reads only the unit's own tile: multiples of 8 at least 3 inside (4 before the far edge)."""
    return [(x, y) for y in range(u["y"] + 8, u["y"] + u["h"] - 4, 8) for x in range(u["x"] + 8, u["x"] + u["w"] - 4, 8)]


# ---------------------------------------------------------------------------------------------------------------- digests

def picture_names():
    return REGULAR + AFFINE + GPM + CIIP + SAO + ALF + ALF_CC


def inter_digests(name, run):
    pic, _ = inter_picture(name)
    out = run(pic)
    rec = {"inputs": ic.inputs_digest(pic), **ic.plane_digests(out.planes)}
    if "R" in pic.kinds:
        rec["dmvr"] = ic.sha(ic.mvf_bytes(out.dmvr))
    return rec


def host_digests(lib, side, name):
    """The record of ref_extremes.json for one picture, computed on the host by `side` ("ref" / "orc")."""
    if name in SAO + ALF + ALF_CC:
        return filter_digests(name, lambda fp, s: pc.run_filter(lib, side, fp, s))
    if name in CIIP:
        return ciip_digests(name, lambda cp: ic.run_ciip(lib, side, cp))
    return inter_digests(name, lambda pic: ic.run_picture(lib, side, pic))


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]

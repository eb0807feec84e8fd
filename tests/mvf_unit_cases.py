"""Records, pictures and expectations for vvc355_mvf_unit_pass (the MvField table from one 64-byte record per prediction unit):

* the record builders (plain / affine / gpm) and the grouping per CTU;
* `rule`: the record predicate of include/vvc_mi355.h restated (the CPU test holds it to vvc355_mvf_unit_check);
* `expect_table` / `expect_affine_cus`: the three storage rules restated in numpy, per unit over all of its 4x4 blocks at once;
* `scalar_unit`: a scalar Python loop that follows ff_vvc_store_sb_mvs / ff_vvc_store_gpm_mvf (libavcodec/vvc/vvc_mvs.c:282-491) line by
  line with unbounded integers, and records the largest magnitude an `int` of the reference would have held;
* `expand`: a record list as the vvc355_mv_rec list vvc355_tab_fill_pass takes (the parent's path);
* the case lists of the CPU and GPU tests, and the device run.
Used by the tests and tools/mvf_unit_time.py."""
import ctypes

import numpy as np

from ffvvc_amd import abi, batch

SEED = 0x5EED4D56
PLAIN, AFFINE, GPM = abi.MVF_PLAIN, abi.MVF_AFFINE, abi.MVF_GPM
NONE = abi.MVF_LINK_NONE
MVF_DT = np.dtype([("mv", "<i4", (2, 2)), ("ref_idx", "i1", (2,)), ("hpel_if_idx", "u1"), ("bcw_idx", "u1"), ("pred_flag", "u1"), ("ciip_flag", "u1"),
                   ("pad_", "u1", (2,))])
UNIT_DT = np.dtype([("x0", "<i2"), ("y0", "<i2"), ("w", "u1"), ("h", "u1"), ("kind", "u1"), ("aux", "u1"), ("link", "<u4"), ("pf", "u1"),
                    ("ref_idx", "i1", (2,)), ("pad_", "u1"), ("body", "<i4", (12,))])
MV_REC_DT = np.dtype([("x0", "<i2"), ("y0", "<i2"), ("w", "u1"), ("h", "u1"), ("pad_", "u1", (2,)), ("mvf", "V24")])
CU_DT = np.dtype(abi.AffineCu, align=True)
assert MVF_DT.itemsize == 24 and UNIT_DT.itemsize == 64 and MV_REC_DT.itemsize == 32 and CU_DT.itemsize == 144
MV_MIN, MV_MAX = -(1 << 17), (1 << 17) - 1

# the GPM partition tables (vvc_data.c, H.266 tables 36 and 37): angleIdx / distanceIdx per partition and disLut
GPM_ANGLE = np.array([0, 0, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 8, 8, 11, 11, 11, 11, 12, 12, 12, 12, 13, 13, 13, 13,
                      14, 14, 14, 14, 16, 16, 18, 18, 18, 19, 19, 19, 20, 20, 20, 21, 21, 21, 24, 24, 27, 27, 27, 28, 28, 28, 29, 29, 29, 30, 30, 30])
GPM_DISTANCE = np.array([1, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 1, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3,
                         0, 1, 2, 3, 1, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3])
GPM_DIS_LUT = np.array([8, 8, 8, 8, 4, 4, 2, 1, 0, -1, -2, -4, -4, -8, -8, -8, -8, -8, -8, -8, -4, -4, -2, -1, 0, 1, 2, 4, 4, 8, 8, 8])
AFFINE_SHAPES = [(w, h) for w in (8, 16, 32, 64, 128) for h in (8, 16, 32, 64, 128)]
GPM_SHAPES = sorted((w, h) for w in (8, 16, 32, 64) for h in (8, 16, 32, 64) if w < 8 * h and h < 8 * w)
assert len(AFFINE_SHAPES) == 25 and len(GPM_SHAPES) == 14


class Geo:
    def __init__(self, width, height, ctb_log2):
        self.width, self.height, self.ctb_log2 = width, height, ctb_log2
        ctb = 1 << ctb_log2
        self.cw, self.ch = (width + ctb - 1) // ctb, (height + ctb - 1) // ctb
        self.tw, self.th = width // 4, height // 4


# ------------------------------------------------------------------------------------------------------------------------- records

def mvfield(mv=((0, 0), (0, 0)), ref_idx=(0, 0), hpel=0, bcw=0, pred_flag=0, ciip=0, pad=(0, 0)):
    m = np.zeros((), MVF_DT)
    m["mv"], m["ref_idx"], m["hpel_if_idx"], m["bcw_idx"], m["pred_flag"], m["ciip_flag"], m["pad_"] = mv, ref_idx, hpel, bcw, pred_flag, ciip, pad
    return m


def _unit(x, y, w, h, kind, aux=0, link=0, pf=0, ref_idx=(0, 0), body=b""):
    r = np.zeros((), UNIT_DT)
    r["x0"], r["y0"], r["w"], r["h"], r["kind"], r["aux"], r["link"], r["pf"], r["ref_idx"] = x, y, w, h, kind, aux, link, pf, ref_idx
    r["body"] = np.frombuffer(body.ljust(48, b"\0"), "<i4")
    return r


def plain(x, y, w, h, m):
    return _unit(x, y, w, h, PLAIN, body=m.tobytes())


def affine(x, y, w, h, model, pred, cp, ref_idx=(0, 0), hpel=0, bcw=0, link=NONE):
    """cp[list][control point][x, y]"""
    return _unit(x, y, w, h, AFFINE, model, link, pred | hpel << 2 | bcw << 4, ref_idx, np.asarray(cp, "<i4").reshape(12).tobytes())


def gpm(x, y, w, h, part, m0, m1):
    return _unit(x, y, w, h, GPM, part, body=m0.tobytes() + m1.tobytes())


def group(g, units):
    """(records ordered by the CTU of their origin, ctu_first): the grouping a parser produces."""
    units = np.array(units, UNIT_DT) if not isinstance(units, np.ndarray) else units
    rs = (units["y0"].astype(np.int64) >> g.ctb_log2) * g.cw + (units["x0"].astype(np.int64) >> g.ctb_log2)
    order = np.argsort(rs, kind="stable")
    return np.ascontiguousarray(units[order]), np.searchsorted(rs[order], np.arange(g.cw * g.ch + 1)).astype(np.int32)


def ctu_of(first, n):
    """The CTU each of n records is filed under (-1: in no CTU's range), with the pass's clamping of a range."""
    out = np.full(n, -1, np.int64)
    for rs in range(len(first) - 1):
        r0 = min(max(int(first[rs]), 0), n)
        r1 = min(max(int(first[rs + 1]), r0), min(n, r0 + 65535))
        out[r0:r1] = rs
    return out


def rule(g, r, rs, n_affine_cus):
    """include/vvc_mi355.h: 0, or the abi.MVF_UNIT_R_* of the first rule record r breaks when filed under CTU rs."""
    x0, y0, w, h, kind, aux = (int(r[k]) for k in ("x0", "y0", "w", "h", "kind", "aux"))
    ctb = 1 << g.ctb_log2
    ox, oy = (rs % g.cw) * ctb, (rs // g.cw) * ctb
    if not w or not h or (w | h) & 3 or w > 128 or h > 128:
        return abi.MVF_UNIT_R_SIDE
    if x0 < 0 or y0 < 0 or (x0 | y0) & 3 or x0 + w > g.width or y0 + h > g.height:
        return abi.MVF_UNIT_R_PLACE
    if x0 < ox or y0 < oy or x0 + w > ox + ctb or y0 + h > oy + ctb:
        return abi.MVF_UNIT_R_CTU
    if int(r["pad_"]):
        return abi.MVF_UNIT_R_PAD
    if kind > GPM:
        return abi.MVF_UNIT_R_KIND
    if kind == AFFINE:
        if w < 8 or h < 8 or w & (w - 1) or h & (h - 1):
            return abi.MVF_UNIT_R_AFF_SHAPE
        if aux not in (1, 2):
            return abi.MVF_UNIT_R_AFF_MODEL
        if not int(r["pf"]) & 3:
            return abi.MVF_UNIT_R_AFF_PRED
        if int(r["link"]) != NONE and int(r["link"]) >= n_affine_cus:
            return abi.MVF_UNIT_R_AFF_LINK
    elif kind == GPM:
        if not (8 <= w <= 64 and 8 <= h <= 64):
            return abi.MVF_UNIT_R_GPM_SHAPE
        if w >= 8 * h or h >= 8 * w:
            return abi.MVF_UNIT_R_GPM_RATIO
        if aux > 63:
            return abi.MVF_UNIT_R_GPM_PART
        parts = r["body"].view(MVF_DT)
        if int(parts[0]["pred_flag"]) not in (1, 2) or int(parts[1]["pred_flag"]) not in (1, 2):
            return abi.MVF_UNIT_R_GPM_PRED
    return 0


def placed(g, units, first, n_affine_cus):
    """bool per record: the pass writes it."""
    rs = ctu_of(first, len(units))
    return np.array([rs[i] >= 0 and rule(g, units[i], int(rs[i]), n_affine_cus) == 0 for i in range(len(units))], bool)


# ------------------------------------------------------------------------------------------------ the storage rules, in numpy

def round_mv(v, s):
    """ff_vvc_round_mv(., 0, s) on an int64 array (vvc_mvs.c:1739)."""
    return (v + (1 << (s - 1)) - (v >= 0)) >> s


def sb_params(cp, model, w, h):
    """init_subblock_params for one list: cp[3][2] -> (d_hor_x, d_ver_x, d_hor_y, d_ver_y, scale_hor, scale_ver), Python ints."""
    cp = [[int(v) for v in p] for p in cp]
    sw, sh = 1 << (7 - (w.bit_length() - 1)), 1 << (7 - (h.bit_length() - 1))
    d_hor_x, d_ver_x = (cp[1][0] - cp[0][0]) * sw, (cp[1][1] - cp[0][1]) * sw
    if model == 2:
        d_hor_y, d_ver_y = (cp[2][0] - cp[0][0]) * sh, (cp[2][1] - cp[0][1]) * sh
    else:
        d_hor_y, d_ver_y = -d_ver_x, d_hor_x
    return d_hor_x, d_ver_x, d_hor_y, d_ver_y, cp[0][0] * 128, cp[0][1] * 128


def is_fallback(p, bi):
    a, b, c, d = 4 * (2048 + p[0]), 4 * p[2], 4 * (2048 + p[3]), 4 * p[1]
    if bi:
        bw = ((max(0, a, b, a + b) - min(0, a, b, a + b)) >> 11) + 9
        bh = ((max(0, c, d, c + d) - min(0, c, d, c + d)) >> 11) + 9
        return bw * bh > 225
    return not (((abs(a) >> 11) + 9) * ((abs(d) >> 11) + 9) <= 165 and ((abs(b) >> 11) + 9) * ((abs(c) >> 11) + 9) <= 165)


def prof_flag(cp, model, fallback, prof_disabled):
    if prof_disabled or fallback:
        return 0
    same1, same2 = tuple(cp[0]) == tuple(cp[1]), tuple(cp[0]) == tuple(cp[2])
    return int(not same1) if model == 1 else int(not (same1 and same2))


def unit_cp(r):
    return r["body"].astype(np.int64).reshape(2, 3, 2)


def affine_unit(r, prof_disabled=0):
    """(entries[h / 4][w / 4] MVF_DT, prof_flags, diff_mv[2][2][16], facts) of a well-formed AFFINE record; facts per list:
    fallback, flag, the unclipped motion and offsets (for the premises)."""
    w, h, model, pf = int(r["w"]), int(r["h"]), int(r["aux"]), int(r["pf"])
    pred = pf & 3
    e = np.zeros((h // 4, w // 4), MVF_DT)
    e["ref_idx"], e["hpel_if_idx"], e["bcw_idx"], e["pred_flag"] = r["ref_idx"], (pf >> 2) & 3, pf >> 4, pred
    flags, dmv, facts = 0, np.zeros((2, 2, 16), np.int16), {}
    sby, sbx = np.mgrid[0:h // 4, 0:w // 4].astype(np.int64)
    for l in range(2):
        if not pred >> l & 1:
            continue
        cp = unit_cp(r)[l]
        p = sb_params(cp, model, w, h)
        fb = is_fallback(p, pred == 3)
        xp = np.full_like(sbx, w >> 1) if fb else 2 + 4 * sbx
        yp = np.full_like(sby, h >> 1) if fb else 2 + 4 * sby
        raw = np.stack([round_mv(p[4] + p[0] * xp + p[2] * yp, 7), round_mv(p[5] + p[1] * xp + p[3] * yp, 7)], -1)
        e["mv"][:, :, l] = np.clip(raw, MV_MIN, MV_MAX)
        fl = prof_flag(cp.tolist(), model, fb, prof_disabled)
        raw_d = None
        if fl:
            flags |= 1 << l
            y, x = np.mgrid[0:4, 0:4].astype(np.int64)             # index 4 * y + x
            raw_d = np.stack([round_mv(x * (p[0] * 4) + y * (p[2] * 4) - 6 * (p[0] + p[2]), 8),
                              round_mv(x * (p[1] * 4) + y * (p[3] * 4) - 6 * (p[1] + p[3]), 8)]).reshape(2, 16)
            dmv[l] = np.clip(raw_d, -31, 31)
        facts[l] = dict(fallback=fb, flag=fl, raw=raw, raw_d=raw_d, pre=(p[4] + p[0] * xp + p[2] * yp, p[5] + p[1] * xp + p[3] * yp))
    return e, flags, dmv, facts


def gpm_types(w, h, part):
    """(s_type[h / 4][w / 4], is_flip, shift_hor) of ff_vvc_store_gpm_mvf."""
    angle, distance = int(GPM_ANGLE[part]), int(GPM_DISTANCE[part])
    disp_x, disp_y = int(GPM_DIS_LUT[angle]), int(GPM_DIS_LUT[(angle + 8) % 32])
    is_flip = int(13 <= angle <= 27)
    shift_hor = 0 if (angle % 16 == 8 or (angle % 16 and h >= w)) else 1
    sign = 1 if angle < 16 else -1
    off_x, off_y = (-w) >> 1, (-h) >> 1
    if not shift_hor:
        off_y += sign * ((distance * h) >> 3)
    else:
        off_x += sign * ((distance * w) >> 3)
    y, x = np.mgrid[0:h:4, 0:w:4].astype(np.int64)
    motion_idx = ((x + off_x) * 2 + 5) * disp_x + ((y + off_y) * 2 + 5) * disp_y
    s_type = np.where(np.abs(motion_idx) < 32, 2, np.where(motion_idx <= 0, 1 - is_flip, is_flip))
    return s_type, is_flip, shift_hor


def gpm_unit(r):
    """(entries, s_type) of a well-formed GPM record."""
    w, h = int(r["w"]), int(r["h"])
    m0, m1 = r["body"].view(MVF_DT)
    s_type, _, _ = gpm_types(w, h, int(r["aux"]))
    both = m0.copy()
    lx = int(m1["pred_flag"]) - 1
    both["pred_flag"] = 3
    both["ref_idx"][lx] = m1["ref_idx"][lx]
    both["mv"][lx] = m1["mv"][lx]
    bi = (int(m0["pred_flag"]) | int(m1["pred_flag"])) == 3
    e = np.zeros((h // 4, w // 4), MVF_DT)
    e[s_type == 0] = m0
    e[(s_type == 1) | ((s_type == 2) & (not bi))] = m1
    e[(s_type == 2) & bi] = both
    return e, s_type


def unit_entries(r, prof_disabled=0):
    kind, w, h = int(r["kind"]), int(r["w"]), int(r["h"])
    if kind == PLAIN:
        e = np.zeros((h // 4, w // 4), MVF_DT)
        e[:] = r["body"][:6].view(MVF_DT)[0]
        return e
    return affine_unit(r, prof_disabled)[0] if kind == AFFINE else gpm_unit(r)[0]


def expect_table(g, units, first, table, n_affine_cus=0):
    """Write the placed records' entries into `table` (MVF_DT, th rows, >= tw columns) in place; returns the placed mask."""
    ok = placed(g, units, first, n_affine_cus)
    for r in units[ok]:
        x, y, w, h = int(r["x0"]) // 4, int(r["y0"]) // 4, int(r["w"]) // 4, int(r["h"]) // 4
        table[y:y + h, x:x + w] = unit_entries(r)
    return ok


def expect_affine_cus(g, units, first, cus, prof_disabled=0):
    """Write prof_flags and diff_mv of the placed AFFINE records with a link into `cus` (CU_DT) in place."""
    ok = placed(g, units, first, len(cus))
    for r in units[ok]:
        if int(r["kind"]) == AFFINE and int(r["link"]) != NONE:
            _, flags, dmv, _ = affine_unit(r, prof_disabled)
            cus[int(r["link"])]["prof_flags"], cus[int(r["link"])]["diff_mv"] = flags, dmv
    return ok


# ---------------------------------------------------------------------- the reference, line by line, with unbounded integers

class Widest:
    """The largest magnitude the reference would have held in an int."""
    def __init__(self):
        self.v = 0

    def __call__(self, x):
        self.v = max(self.v, abs(x))
        return x


def _round1(v, s, W):
    """ff_vvc_round_mv(., 0, s) on one component, the sum it forms recorded in W."""
    return W(W(v + (1 << (s - 1))) - (1 if v >= 0 else 0)) >> s


def scalar_unit(r, prof_disabled=0, widest=None):
    """ff_vvc_store_sb_mvs (:402-446, with :282-379) / ff_vvc_store_gpm_mvf (:448-491) on one record: ({(x, y): MVF_DT scalar} with x, y
    relative to the unit, cb_prof_flag[2], diff_mv[2][2][16]).  What the reference leaves undefined (the motion and ref_idx of a list not
    in pred_flag, pad) is what the header defines: zero motion, the record's ref_idx."""
    W = widest or Widest()
    cb_width, cb_height = int(r["w"]), int(r["h"])
    out, flags, diff = {}, [0, 0], np.zeros((2, 2, 16), np.int16)
    if int(r["kind"]) == AFFINE:
        model, pf = int(r["aux"]), int(r["pf"])
        pred_flag = pf & 3
        cps = unit_cp(r).tolist()
        params = [None, None]
        for i in range(2):
            if pred_flag & (i + 1):
                cp_mv = cps[i]
                log2_cbw, log2_cbh = cb_width.bit_length() - 1, cb_height.bit_length() - 1          # init_subblock_params
                sp = {}
                sp["d_hor_x"] = W(W(cp_mv[1][0] - cp_mv[0][0]) * (1 << (7 - log2_cbw)))
                sp["d_ver_x"] = W(W(cp_mv[1][1] - cp_mv[0][1]) * (1 << (7 - log2_cbw)))
                if model + 1 == 3:
                    sp["d_hor_y"] = W(W(cp_mv[2][0] - cp_mv[0][0]) * (1 << (7 - log2_cbh)))
                    sp["d_ver_y"] = W(W(cp_mv[2][1] - cp_mv[0][1]) * (1 << (7 - log2_cbh)))
                else:
                    sp["d_hor_y"], sp["d_ver_y"] = -sp["d_ver_x"], sp["d_hor_x"]
                sp["mv_scale_hor"], sp["mv_scale_ver"] = W(cp_mv[0][0] * (1 << 7)), W(cp_mv[0][1] * (1 << 7))
                a, b = W(4 * W(2048 + sp["d_hor_x"])), W(4 * sp["d_hor_y"])                          # is_fallback_mode
                c, d = W(4 * W(2048 + sp["d_ver_y"])), W(4 * sp["d_ver_x"])
                if pred_flag == 3:
                    max_w4, min_w4 = max(0, max(a, max(b, W(a + b)))), min(0, min(a, min(b, a + b)))
                    max_h4, min_h4 = max(0, max(c, max(d, W(c + d)))), min(0, min(c, min(d, c + d)))
                    bx_wx4, bx_hx4 = (W(max_w4 - min_w4) >> 11) + 9, (W(max_h4 - min_h4) >> 11) + 9
                    sp["is_fallback"] = int(W(bx_wx4 * bx_hx4) > 225)
                else:
                    bx_wxh, bx_hxh, bx_wxv, bx_hxv = (abs(a) >> 11) + 9, (abs(d) >> 11) + 9, (abs(b) >> 11) + 9, (abs(c) >> 11) + 9
                    sp["is_fallback"] = 0 if (W(bx_wxh * bx_hxh) <= 165 and W(bx_wxv * bx_hxv) <= 165) else 1
                params[i] = sp
                if prof_disabled or sp["is_fallback"]:                                                # derive_cb_prof_flag_lx
                    flags[i] = 0
                elif model == 1 and cp_mv[0] == cp_mv[1]:
                    flags[i] = 0
                elif model == 2 and cp_mv[0] == cp_mv[1] and cp_mv[0] == cp_mv[2]:
                    flags[i] = 0
                else:
                    flags[i] = 1
                if flags[i]:                                                                          # derive_subblock_diff_mvs
                    pos_offset_x, pos_offset_y = W(6 * W(sp["d_hor_x"] + sp["d_hor_y"])), W(6 * W(sp["d_ver_x"] + sp["d_ver_y"]))
                    for x in range(4):
                        for y in range(4):
                            dx = W(W(W(x * W(sp["d_hor_x"] * 4)) + W(y * W(sp["d_hor_y"] * 4))) - pos_offset_x)
                            dy = W(W(W(x * W(sp["d_ver_x"] * 4)) + W(y * W(sp["d_ver_y"] * 4))) - pos_offset_y)
                            dx, dy = _round1(dx, 8, W), _round1(dy, 8, W)
                            diff[i][0][4 * y + x], diff[i][1][4 * y + x] = min(max(dx, -31), 31), min(max(dy, -31), 31)
        for sby in range(cb_height // 4):
            for sbx in range(cb_width // 4):
                mvf = mvfield(ref_idx=r["ref_idx"], hpel=(pf >> 2) & 3, bcw=pf >> 4, pred_flag=pred_flag)
                for i in range(2):
                    if pred_flag & (i + 1):
                        sp = params[i]
                        x_pos_cb = (cb_width >> 1) if sp["is_fallback"] else 2 + (sbx << 2)
                        y_pos_cb = (cb_height >> 1) if sp["is_fallback"] else 2 + (sby << 2)
                        mx = W(W(sp["mv_scale_hor"] + W(sp["d_hor_x"] * x_pos_cb)) + W(sp["d_hor_y"] * y_pos_cb))
                        my = W(W(sp["mv_scale_ver"] + W(sp["d_ver_x"] * x_pos_cb)) + W(sp["d_ver_y"] * y_pos_cb))
                        mx, my = _round1(mx, 7, W), _round1(my, 7, W)
                        mvf["mv"][i] = (min(max(mx, MV_MIN), MV_MAX), min(max(my, MV_MIN), MV_MAX))
                out[(4 * sbx, 4 * sby)] = mvf
    else:
        part = int(r["aux"])
        gpm_mv = r["body"].view(MVF_DT)
        angle_idx, distance_idx = int(GPM_ANGLE[part]), int(GPM_DISTANCE[part])
        displacement_x, displacement_y = int(GPM_DIS_LUT[angle_idx]), int(GPM_DIS_LUT[(angle_idx + 8) % 32])
        is_flip = int(13 <= angle_idx <= 27)
        shift_hor = 0 if (angle_idx % 16 == 8 or (angle_idx % 16 and cb_height >= cb_width)) else 1
        sign = 1 if angle_idx < 16 else -1
        offset_x, offset_y = (-cb_width) >> 1, (-cb_height) >> 1
        if not shift_hor:
            offset_y += sign * ((distance_idx * cb_height) >> 3)
        else:
            offset_x += sign * ((distance_idx * cb_width) >> 3)
        for y in range(0, cb_height, 4):
            for x in range(0, cb_width, 4):
                motion_idx = W(W(((x + offset_x) * 2 + 5) * displacement_x) + W(((y + offset_y) * 2 + 5) * displacement_y))
                s_type = 2 if abs(motion_idx) < 32 else ((1 - is_flip) if motion_idx <= 0 else is_flip)
                pred_flag = int(gpm_mv[0]["pred_flag"]) | int(gpm_mv[1]["pred_flag"])
                if not s_type:
                    out[(x, y)] = gpm_mv[0].copy()
                elif s_type == 1 or (s_type == 2 and pred_flag != 3):
                    out[(x, y)] = gpm_mv[1].copy()
                else:
                    mvf = gpm_mv[0].copy()
                    lx = int(gpm_mv[1]["pred_flag"]) - 1
                    mvf["pred_flag"] = 3
                    mvf["ref_idx"][lx] = gpm_mv[1]["ref_idx"][lx]
                    mvf["mv"][lx] = gpm_mv[1]["mv"][lx]
                    out[(x, y)] = mvf
    return out, flags, diff


# ----------------------------------------------------------------------------------------------- the parent's path: vvc355_mv_rec

def expand(g, units, first, n_affine_cus=0, merge=True):
    """The placed records as vvc355_mv_rec rectangles of equal motion, grouped per CTU: (records, ctu_first).  A PLAIN unit is one
    rectangle; an AFFINE or GPM unit one per 4x4 block, or (merge) one where all of its blocks came out equal."""
    ok = placed(g, units, first, n_affine_cus)
    out = []
    for r in units[ok]:
        x0, y0, w, h = int(r["x0"]), int(r["y0"]), int(r["w"]), int(r["h"])
        e = unit_entries(r)
        if int(r["kind"]) == PLAIN or (merge and np.all(e == e[0, 0])):
            out.append((x0, y0, w, h, (0, 0), e[0, 0].tobytes()))
        else:
            out += [(x0 + 4 * bx, y0 + 4 * by, 4, 4, (0, 0), e[by, bx].tobytes()) for by in range(h // 4) for bx in range(w // 4)]
    recs = np.array(out, MV_REC_DT) if out else np.zeros(0, MV_REC_DT)
    rs = (recs["y0"].astype(np.int64) >> g.ctb_log2) * g.cw + (recs["x0"].astype(np.int64) >> g.ctb_log2)
    order = np.argsort(rs, kind="stable")
    return np.ascontiguousarray(recs[order]), np.searchsorted(rs[order], np.arange(g.cw * g.ch + 1)).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------- case lists

def rand_mvfield(rng, pred_flag=None, wild=False):
    """A MvField as a parser would hold it; wild: any bytes in the fields the pass only copies (pad included)."""
    pf = int(rng.integers(1, 4)) if pred_flag is None else pred_flag
    m = mvfield(mv=rng.integers(MV_MIN, MV_MAX + 1, size=(2, 2)), ref_idx=rng.integers(0, 3, size=2), hpel=int(rng.integers(0, 2)),
                bcw=int(rng.integers(0, 5)), pred_flag=pf, ciip=int(rng.integers(0, 2)))
    if wild:
        m["pad_"] = rng.integers(1, 256, size=2)
    return m


REGIMES = ("small", "fallback", "equal", "ends")


def rand_cp(rng, regime, w, h, model):
    """cp[2][3][2] within the 18-bit range.  small: deltas of a few units per sub-block; fallback: deltas around the size at which
    is_fallback_mode flips (16 * side per control point) and at which diff_mv reaches +-31; equal: equal control points (for the
    6-parameter model sometimes only the first two); ends: control points at and next to the ends of the range."""
    cp = np.zeros((2, 3, 2), np.int64)
    for l in range(2):
        if regime == "ends":
            edge = int(rng.choice([MV_MIN, MV_MAX]))
            base = np.array([edge, int(rng.choice([MV_MIN, MV_MAX]))]) if rng.random() < 0.5 else np.array([edge, int(rng.integers(-4000, 4000))])
            cp[l, 0] = base
            for k in (1, 2):
                far = rng.random() < 0.3
                cp[l, k] = rng.integers(MV_MIN, MV_MAX + 1, size=2) if far else base + rng.integers(-(w + h), w + h + 1, size=2)
        else:
            cp[l, 0] = rng.integers(-3000, 3001, size=2)
            if regime == "small":
                cp[l, 1] = cp[l, 0] + rng.integers(-(w // 2), w // 2 + 1, size=2)
                cp[l, 2] = cp[l, 0] + rng.integers(-(h // 2), h // 2 + 1, size=2)
            elif regime == "fallback":
                cp[l, 1] = cp[l, 0] + rng.integers(-28 * w, 28 * w + 1, size=2) * np.array([1, int(rng.integers(0, 2))])
                cp[l, 2] = cp[l, 0] + rng.integers(-28 * h, 28 * h + 1, size=2) * np.array([int(rng.integers(0, 2)), 1])
            else:
                cp[l, 1] = cp[l, 0]
                cp[l, 2] = cp[l, 0] if rng.random() < 0.6 else cp[l, 0] + rng.integers(-h, h + 1, size=2)
    if model == 1:
        cp[:, 2] = rng.integers(-99, 100, size=(2, 2))           # never read by the 4-parameter model
    return np.clip(cp, MV_MIN, MV_MAX)


def affine_params(w, h, seed_extra=0):
    """The affine sweep for one shape: [(model, pred, regime, rep)] x control points; both models x pred_flag 1 / 2 / 3 x four regimes."""
    rng = np.random.default_rng(SEED + 1000 * w + h + seed_extra)
    reps = 3 if w * h <= 1024 else 1
    out = []
    for model in (1, 2):
        for pred in (1, 2, 3):
            for regime in REGIMES:
                for _ in range(reps):
                    ref_idx = [int(rng.integers(0, 3)) if pred >> l & 1 else -1 for l in range(2)]
                    out.append(dict(model=model, pred=pred, regime=regime, cp=rand_cp(rng, regime, w, h, model), ref_idx=ref_idx,
                                    hpel=int(rng.integers(0, 2)), bcw=int(rng.integers(0, 5)) if pred == 3 else 0))
    return out


def gpm_params(w, h):
    """The GPM sweep for one shape: 64 partitions x the four list combinations of the two parts."""
    rng = np.random.default_rng(SEED + 7 + 1000 * w + h)
    return [dict(part=part, m0=rand_mvfield(rng, l0 + 1, wild=True), m1=rand_mvfield(rng, l1 + 1, wild=True))
            for part in range(64) for l0 in range(2) for l1 in range(2)]


def pack(shape, width, height, ctb_log2, make, params):
    """Units of one shape in slots of pictures of the given size: [(Geo, units, first)], as many pictures as the list needs.  make(x, y, p, i)
    -> record i at (x, y)."""
    w, h = shape
    g = Geo(width, height, ctb_log2)
    ctb = 1 << ctb_log2
    slots = [(x, y) for y in range(0, height - h + 1, h) for x in range(0, width - w + 1, w) if x // ctb == (x + w - 1) // ctb and y // ctb == (y + h - 1) // ctb]
    pics = []
    for k in range(0, len(params), len(slots)):
        chunk = params[k:k + len(slots)]
        units = [make(x, y, p, i) for i, ((x, y), p) in enumerate(zip(slots, chunk))]
        pics.append((g,) + group(g, units))
    return pics


def affine_pictures(shape):
    """The shape's sweep as pictures (256 x 128 at the smallest CTU that holds the shape), every unit linked to its own vvc355_affine_cu."""
    w, h = shape
    ctb_log2 = max(5, max(w, h).bit_length() - 1)
    return pack(shape, 256, 128, ctb_log2,
                lambda x, y, p, i: affine(x, y, w, h, p["model"], p["pred"], p["cp"], p["ref_idx"], p["hpel"], p["bcw"], link=i), affine_params(w, h))


def gpm_pictures(shape):
    w, h = shape
    ctb_log2 = max(5, max(w, h).bit_length() - 1)
    return pack(shape, 256, 192, ctb_log2, lambda x, y, p, i: gpm(x, y, w, h, p["part"], p["m0"], p["m1"]), gpm_params(w, h))


def plain_picture(ctb_log2, width=136, height=72, modes=None):
    """A picture tiled with PLAIN units, CTU rs in mode modes[rs % len(modes)]: 0 = one unit, the largest the CTU allows inside the picture;
    1 = 4x4 units; 2 = 4x8, 8x4 and 4x4 units.  MvFields with any bytes, intra units among them."""
    rng = np.random.default_rng(SEED + 50 + ctb_log2 + width)
    g = Geo(width, height, ctb_log2)
    ctb = 1 << ctb_log2
    units = []
    for rs in range(g.cw * g.ch):
        ox, oy = (rs % g.cw) * ctb, (rs // g.cw) * ctb
        cw_, ch_ = min(ctb, width - ox), min(ctb, height - oy)
        modes = modes or ((0, 2) if g.cw * g.ch < 3 else (0, 1, 2))
        mode = modes[rs % len(modes)]
        if mode == 0:
            units.append(plain(ox, oy, cw_, ch_, rand_mvfield(rng, wild=True)))
        elif mode == 1:
            units += [plain(ox + x, oy + y, 4, 4, rand_mvfield(rng, wild=True)) for y in range(0, ch_, 4) for x in range(0, cw_, 4)]
        else:
            for y in range(0, ch_, 8):
                for x in range(0, cw_, 8):
                    if y + 8 > ch_ or x + 8 > cw_ or (x + y) % 24 == 8:
                        units += [plain(ox + x + dx, oy + y + dy, 4, 4, rand_mvfield(rng, wild=True)) for dy in range(0, min(8, ch_ - y), 4)
                                  for dx in range(0, min(8, cw_ - x), 4)]
                    elif (x + y) % 16:
                        units += [plain(ox + x, oy + y, 4, 8, rand_mvfield(rng)), plain(ox + x + 4, oy + y, 4, 8, mvfield())]      # the second: intra
                    else:
                        units += [plain(ox + x, oy + y, 8, 4, rand_mvfield(rng)), plain(ox + x, oy + y + 4, 8, 4, rand_mvfield(rng, wild=True))]
    return (g,) + group(g, units)


def mixed_picture(leaves, width=200, height=136, ctb_log2=6, seed=0):
    """A picture whose units are `leaves` ((x, y, w, h), inside their CTUs), each of a kind its shape allows; AFFINE units are linked
    in order.  Returns (Geo, units, first, n_affine_cus)."""
    rng = np.random.default_rng(SEED + 900 + seed)
    g = Geo(width, height, ctb_log2)
    units, n_aff = [], 0
    for (x, y, w, h) in leaves:
        pow2 = not (w & (w - 1)) and not (h & (h - 1))
        opts = [PLAIN] + ([AFFINE] * 2 if pow2 and w >= 8 and h >= 8 else []) + ([GPM] * 2 if (w, h) in GPM_SHAPES else [])
        kind = int(rng.choice(opts))
        if kind == PLAIN:
            units.append(plain(x, y, w, h, rand_mvfield(rng) if rng.random() < 0.8 else mvfield()))
        elif kind == AFFINE:
            model, pred = int(rng.integers(1, 3)), int(rng.integers(1, 4))
            cp = rand_cp(rng, REGIMES[int(rng.integers(0, 3))], w, h, model)
            units.append(affine(x, y, w, h, model, pred, cp, [int(rng.integers(0, 3)) if pred >> l & 1 else -1 for l in range(2)],
                                int(rng.integers(0, 2)), int(rng.integers(0, 5)) if pred == 3 else 0, link=n_aff))
            n_aff += 1
        else:
            units.append(gpm(x, y, w, h, int(rng.integers(0, 64)), rand_mvfield(rng, int(rng.integers(1, 3))), rand_mvfield(rng, int(rng.integers(1, 3)))))
    return (g,) + group(g, units) + (n_aff,)


# ------------------------------------------------------------------------------ the pin from the reference (tests/golden/mvf_unit_ref.json)

def ref_groups():
    """{name: [(record at (0, 0), prof_disabled)]}: per affine shape every unit of the sweep with PROF allowed and switched off, per GPM
    shape every unit of the sweep.  What the reference's ff_vvc_store_sb_mvs / ff_vvc_store_gpm_mvf were run on for the fixture."""
    out = {}
    for kind, shapes, pictures in (("A", AFFINE_SHAPES, affine_pictures), ("G", GPM_SHAPES, gpm_pictures)):
        for shape in shapes:
            units = np.concatenate([u for _, u, _ in pictures(shape)]).copy()
            units["x0"], units["y0"], units["link"] = 0, 0, NONE if kind == "A" else 0
            out[f"{kind}{shape[0]}x{shape[1]}"] = [(r, d) for d in ((0, 1) if kind == "A" else (0,)) for r in units]
    return out


def ref_inputs(cases):
    return b"".join(r.tobytes() + np.int32(d).tobytes() for r, d in cases)


def ref_outputs(cases):
    """What the fixture's digests are taken of, from the numpy side: per case the unit's entries in raster order (of an AFFINE unit with
    motion and ref_idx of a list not in pred_flag zeroed, which the reference leaves undefined; pad bytes zeroed), cb_prof_flag[2] as two
    bytes, diff_mv[2][2][16] (zeros where the flag is 0; all zeros for GPM)."""
    out = []
    for r, d in cases:
        if int(r["kind"]) == AFFINE:
            e, flags, dmv, _ = affine_unit(r, d)
            for l in range(2):
                if not int(r["pf"]) >> l & 1:
                    e["ref_idx"][:, :, l] = 0
        else:
            e, flags, dmv = gpm_unit(r)[0].copy(), 0, np.zeros((2, 2, 16), np.int16)
        e["pad_"] = 0
        out.append(e.tobytes() + bytes([flags & 1, flags >> 1]) + dmv.tobytes())
    return b"".join(out)


# ------------------------------------------------------------------------------------------------------------------- the device

def unit_frame(g, units_ptr, n_units, first_ptr, mvf_ptr, pitch, cus_ptr=0, n_cus=0, prof_disabled=0):
    f = abi.MvfUnitFrame()
    f.units, f.ctu_first, f.mvf, f.affine_cus = units_ptr, first_ptr, mvf_ptr, cus_ptr
    f.n_units, f.n_affine_cus, f.mvf_pitch = n_units, n_cus, pitch
    f.width, f.height, f.ctb_width, f.ctb_height, f.ctb_log2, f.prof_disabled = g.width, g.height, g.cw, g.ch, g.ctb_log2, prof_disabled
    return f


def sentinel_table(g, pitch=None, rows_extra=1):
    """A table allocation of th + rows_extra rows of `pitch` entries, every byte 0xEE."""
    t = np.zeros((g.th + rows_extra, pitch or g.tw), MVF_DT)
    t.view(np.uint8)[:] = 0xEE
    return t


def sentinel_cus(n):
    c = np.zeros(n, CU_DT)
    c.view(np.uint8)[:] = 0xDD
    return c


class DeviceRun:
    """The pass's inputs and outputs on the device: `table` (and `cus`) are uploaded as they are, issue() launches, download() fetches both."""

    def __init__(self, dev, g, units, first, table, cus=None, prof_disabled=0, n_cus=None):
        self.dev, self.table, self.cus = dev, table, cus
        self.d_units = batch.DeviceBuffer.from_host(units.view(np.uint8) if len(units) else np.zeros(64, np.uint8))
        self.d_first = batch.DeviceBuffer.from_host(first)
        self.d_tab = batch.DeviceBuffer.from_host(table.view(np.uint8))
        self.d_cus = batch.DeviceBuffer.from_host(cus.view(np.uint8)) if cus is not None and len(cus) else None
        self.f = unit_frame(g, self.d_units.ptr, len(units), self.d_first.ptr, self.d_tab.ptr, table.shape[1], self.d_cus.ptr if self.d_cus else 0,
                            (len(cus) if cus is not None else 0) if n_cus is None else n_cus, prof_disabled)
        self.d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.f), np.uint8))

    def issue(self, stream=None):
        return self.dev.vvc355_mvf_unit_pass(stream, self.d_f.ptr, ctypes.addressof(self.f))

    def download(self):
        got = self.d_tab.to_host(np.uint8, (self.table.nbytes,)).view(MVF_DT).reshape(self.table.shape)
        return got, (self.d_cus.to_host(np.uint8, (self.cus.nbytes,)).view(CU_DT) if self.d_cus else self.cus)


def run_device(dev, g, units, first, table, cus=None, prof_disabled=0, n_cus=None):
    """The pass on copies of `table` (and `cus`): (table, cus, return code) as they come back."""
    run = DeviceRun(dev, g, units, first, table, cus, prof_disabled, n_cus)
    rc = run.issue()
    dev.vvc355_stream_sync(None)
    return run.download() + (rc,)


def table_mismatch(got, want):
    """'' or a line naming the first entry whose 24 bytes differ."""
    a, b = got.view(np.uint8).reshape(got.shape + (24,)), want.view(np.uint8).reshape(want.shape + (24,))
    bad = np.argwhere(np.any(a != b, axis=-1))
    if not len(bad):
        return ""
    r, c = bad[0]
    return f"{len(bad)} entries differ, first at (row, col) ({r}, {c}): got {got[r, c]}, want {want[r, c]}"


def cus_mismatch(got, want):
    a, b = got.view(np.uint8).reshape(-1, CU_DT.itemsize), want.view(np.uint8).reshape(-1, CU_DT.itemsize)
    bad = np.argwhere(a != b)
    if not len(bad):
        return ""
    u, o = bad[0]
    return f"{len(bad)} bytes of the affine records differ, first byte {o} of record {u}: got {a[u, o]}, want {b[u, o]}"

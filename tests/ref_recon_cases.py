"""Pictures for the RECON walk and the TB record passes pinned against the reference's own caller (oracle/ref_shim_intra.c:
ref_recon_picture = ff_vvc_reconstruct per CTU on real contexts).  ONE unit-level description per picture — coding units in decoding order
per CTU, their transform units and transform blocks with int32 levels — is the single source; two things are derived from it:

  (a) shim_arrays(): the plain arrays ref_recon_picture builds CodingUnit / TransformUnit lists and the parser's tables from;
  (b) derive(): the project's inputs by the rules INTEGRATION.md section 3 states — per-CTU command lists (MARK / PRED / CCLM / RESID, one
      command per reference call in the reference's order) with the LIGHT / LUMA_LEFT / LUMA_UP flags, vvc355_intra_tu / vvc355_ts_tu /
      vvc355_inter_tu specs in the form of intra_tb_cases / ts_tb_cases / inter_tb_cases (grouped as the passes demand, tb->qp by derive_qp's
      clip, KEEP and the unit bits), which chroma residuals of inter units stay with the walk (their unit's luma neighbour lies in a CTU the
      walk writes), and the vvc355_lmcs_scale_frame.

oracle_side() feeds (b) to the existing oracle pieces: intra_tb_cases.oracle_block, ts_tb_cases.residual_of (the residual of the inter_tb_cases
and ts_tb_cases walks), their add / scaled add / joint add tail in those walks' order (luma, orc_lmcs_vpdu_scale_pass on the picture's own slice
and tile maps, chroma), then orc_recon_frame_pass.  Those modules are imported, never changed.  Used by tests/test_ref_recon_cpu.py,
tests/test_ref_recon_gpu.py and tools/gen_golden.py; tests/golden/ref_recon.json holds the digests.

Every picture is deterministic, at most 264x136, and starts from bipred_cases.smooth_picture planes, which stand for the inter prediction.
draw() has hooks for other content, levels, unit kinds, modes and LMCS models (tests/recon_extreme_cases.py draws its worst-case pictures
through them); unset, as for every picture listed or swept here, they leave the draw as it was, random stream included.
Domain (what the generator draws; the shim returns -1 outside what its objects can hold and the tests fail on that): no CIIP unit (the CIIP
command stays pinned through put_ciip and ref_inter_cases I0-I4), no scaling lists, act_enabled_flag 0, intra units at most 64x64, no intra
chroma block under 4 samples wide or under 16 samples (the standard has none; the reference's predictors write 4 columns there, past the
block, so units that small are inter units here, down to 4x4), and the two limits of the reference's dequant, asserted in _levels():
tb->qp + (dep_quant && !ts) <= 75 and |level| * scale * 16 + bd_offset < 2^31 (for BDPCM blocks: of the accumulated level).

Sensitivity, checked on the CPU (one misreading of the contract applied to derive() alone, MISREADINGS; listed pictures whose oracle side then
no longer matches the reference; test_ref_recon_cpu.py asserts the table):
  the scale of a scaled chroma block taken from the block's own 64x64 unit, not the coding unit's origin    T2 (its 128-wide inter units)
  no MARK for a unit with coded_flag 0                                                                       T1 T2 T3 T5 T6 T8 T9
  ISP prediction on every part of 1 or 2 samples width                                                       T0-T9
  ph_joint_cbcr_sign_flag dropped                                                                            T2 T4 T5 (the pictures that set it)
"""
import ctypes
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np

import bipred_cases as bc
import intra_tb_cases as itc
import inter_tb_cases as tc
import levels_cases as lc
import recon_cases
import ts_tb_cases as ts
from ffvvc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_recon.json")
SEED = 0x2EC04000
FMT = {0: (1, 1), 1: (1, 1), 2: (1, 0), 3: (0, 0)}           # chroma_format_idc -> (hs, vs); 4:0:0 has no chroma, the shifts are unused
CMD, CTU = recon_cases.CMD, recon_cases.CTU
_cmd = recon_cases.ReconWork._cmd
MAX_TB_QP = 74                              # tb->qp + dep_quant <= 75: where the reference's rem6 / div6 tables end

# name -> what the generator draws.  tools: probabilities of the unit-level draws (see DEFAULT_TOOLS)
_LISTED = {
    # all intra, every tool of the intra path, three slices with differing dep-quant / LMCS flags, partial CTUs right and below
    "T0": dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), intra=1.0, slices=[(1, 1), (0, 0), (1, 1)], lmcs=True),
    # 8 bit 4:4:4, CTU 32 (size_y 32), tiles and wavefront, chroma direct MIP, BDPCM chroma, mixed intra / inter
    "T1": dict(bd=8, idc=3, ctb_log2=5, size=(136, 104), intra=0.5, tiles=True, wpp=1, slices=[(0, 1), (1, 1)], lmcs=True, explicit_mts=True),
    # 12 bit 4:2:2 at transform range 18, CTU 128, inter units of 128 with chroma in the second 64x64 unit, whole inter CTUs
    "T2": dict(bd=12, idc=2, ctb_log2=7, size=(264, 136), intra=0.35, rbits=18, slices=[(1, 1)], lmcs=True, big_inter=True, inter_ctu=0.4, joint_sign=1),
    # 4:0:0
    "T3": dict(bd=10, idc=0, ctb_log2=6, size=(136, 72), intra=0.6, min_cu=4, slices=[(0, 0), (1, 0)], explicit_mts=True),
    # dual-tree all-intra picture
    "T4": dict(bd=10, idc=1, ctb_log2=6, size=(136, 136), intra=1.0, dual=True, min_cu=4, angular=22, slices=[(1, 1)], lmcs=True, collocated=1, joint_sign=1),
    # mostly inter CTUs around a few intra ones: LIGHT CTUs, inter residuals inside intra CTUs, slice and tile edges, explicit MTS, SBT, inter
    # units down to 4x4 whose chroma blocks of four samples stay unscaled
    "T5": dict(bd=10, idc=1, ctb_log2=6, size=(264, 136), intra=0.5, inter_ctu=0.55, min_cu=4, tiles=True, slices=[(1, 1), (0, 1), (1, 0)],
               lmcs=True, explicit_mts=True, joint_sign=1),
    # 12 bit 4:4:4 at range 15 with units down to 4x4: ISP parts 1 and 2 wide, LFNST on 4x4 blocks
    "T6": dict(bd=12, idc=3, ctb_log2=5, size=(72, 72), intra=0.8, min_cu=4, slices=[(0, 1)], lmcs=True, tools=dict(isp=0.5)),
    # 8 bit 4:2:0, CTU 128, all intra with min_qp_prime_ts 2 and no MTS at all
    "T7": dict(bd=8, idc=1, ctb_log2=7, size=(200, 136), intra=1.0, slices=[(0, 0), (1, 1)], lmcs=True, mts=False, min_qp_prime_ts=2, wpp=1, angular=44),
    # the two pictures the older job path can express as well (OLD_PATH): one slice, one tile, no joint Cb-Cr, no unit above 64
    "T8": dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), intra=0.4, inter_ctu=0.4, slices=[(1, 1)], lmcs=True, tools=dict(joint=0.0)),
    "T9": dict(bd=8, idc=2, ctb_log2=5, size=(136, 104), intra=0.5, slices=[(0, 0)], explicit_mts=True, tools=dict(joint=0.0)),
}
OLD_PATH = ["T8", "T9"]
DEFAULT_TOOLS = dict(isp=0.2, mip=0.12, ref_line=0.25, bdpcm=0.12, cclm=0.3, lfnst=0.25, ts=0.12, joint=0.3, sbt=0.25, mts=0.5, coded=0.75,
                     cu_coded=0.85)

MISREADINGS = ("scale_from_block_unit", "no_mark_for_uncoded_unit", "isp_prediction_on_every_part", "joint_sign_dropped")
# which listed pictures each misreading makes differ from the reference (test_ref_recon_cpu.py recomputes and compares)
SENSITIVITY = {
    "scale_from_block_unit": ["T2"],
    "no_mark_for_uncoded_unit": ["T1", "T2", "T3", "T5", "T6", "T8", "T9"],
    "isp_prediction_on_every_part": ["T0", "T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8", "T9"],
    "joint_sign_dropped": ["T2", "T4", "T5"],
}

LEVEL_SCALE = ((40, 45, 51, 57, 64, 72), (57, 64, 72, 80, 90, 102))
DIAG4 = itc.DIAG4


def px(bd):
    return np.uint8 if bd == 8 else np.uint16


# ---------------------------------------------------------------------------------------------------------------- drawing a picture

def _split(rng, x, y, w, h, W, H, min_side, out, big):
    """Random quad / binary partition of a CTU into power-of-two units inside the picture (sizes are multiples of 8; forced splits may go down
    to 8).  Units above 64 a side stay whole only with `big` (128x128, 128x64, 64x128: every 64x64 unit contiguous in coding order)."""
    if x >= W or y >= H:
        return
    inside = x + w <= W and y + h <= H
    floor = min_side if inside else min(min_side, 8)
    must = not inside or ((w > 64 or h > 64) and not (big and rng.random() < 0.6))
    if not must and (max(w, h) <= floor or rng.random() >= (0.8 if max(w, h) > 16 else 0.4)):
        out.append((x, y, w, h))
        return
    can_q = w == h and w >= 2 * floor
    kind = int(rng.integers(0, 3))
    if not inside:
        kind = 0 if can_q else (1 if x + w > W else 2)
    elif w > 64 or h > 64:
        kind = 0 if (w == h and rng.random() < 0.5) else (1 if w > h else 2 if h > w else int(rng.integers(1, 3)))
    if kind == 0 and can_q:
        for dy in (0, h // 2):
            for dx in (0, w // 2):
                _split(rng, x + dx, y + dy, w // 2, h // 2, W, H, min_side, out, big)
    elif (kind == 1 or h <= floor) and w > floor:
        for dx in (0, w // 2):
            _split(rng, x + dx, y, w // 2, h, W, H, min_side, out, big)
    elif h > floor:
        for dy in (0, h // 2):
            _split(rng, x, y + dy, w, h // 2, W, H, min_side, out, big)
    else:
        out.append((x, y, w, h))


def tr_kinds(pic, cu, c_idx, w, h):
    """derive_transform_type restated for ONE purpose, the zero-out that bounds a block's level window: (horizontal, vertical) is DCT-2."""
    isp = cu["isp_type"] != 0
    if c_idx or (isp and cu["lfnst_idx"]):
        return True, True
    implicit = pic.mts_enabled and (isp or (cu["sbt_flag"] and max(w, h) <= 32) or
                                    (not pic.explicit_mts_intra and cu["pred_mode"] == 1 and not cu["lfnst_idx"] and not cu["mip_flag"]))
    if implicit:
        if cu["sbt_flag"]:
            return False, False
        return not 4 <= w <= 16, not 4 <= h <= 16
    return cu["mts_idx"] == 0, cu["mts_idx"] == 0


def tb_qp(pic, cu, tu, c_idx, tsf):
    """derive_qp (vvc_intra.c:277-310): the clip INTEGRATION.md documents for the records' qp."""
    off = 6 * (pic.bd - 8)
    if c_idx == 0:
        qp = cu["qp"][0] + off
    else:
        qp = cu["qp"][3 if (tu["joint"] and tu["coded"][1] and tu["coded"][2]) else c_idx]
    return int(np.clip(qp, 4 + 6 * pic.min_qp_prime_ts if tsf else 0, 63 + off))


def _level_limit(pic, lw, lh, qp, dep, tsf):
    """The largest |level| the reference's signed product holds: |level| * scale * 16 + bd_offset < 2^31."""
    rect = 0 if tsf else (lw + lh) & 1
    q = qp + (1 if dep and not tsf else 0)
    assert q <= MAX_TB_QP + 1, "tb->qp + dep_quant beyond the reference's rem6 / div6 tables"
    scale = LEVEL_SCALE[rect][q % 6] << (q // 6)
    shift = 10 if tsf else pic.bd + rect + (lw + lh) // 2 + 10 - pic.rbits + dep
    assert shift >= 1
    return ((1 << 31) - 1 - ((1 << shift) >> 1)) // (scale * 16)


def _hooked_levels(pic, drawn, w, h, lim, tsf, bdpcm, vert, lfnst, dct2):
    """What a levels= hook returned, held to the domain _levels() draws in: nothing is clipped or repaired here, a hook that leaves it fails."""
    c, nzw, nzh = drawn
    c = np.ascontiguousarray(c, np.int32)
    assert c.shape == (h, w) and c.any() and np.abs(c.astype(np.int64)).max() <= lim, "a levels= hook left the dequant limit"
    if lfnst:
        allowed = np.zeros((h, w), bool)
        for (x, y) in DIAG4[:itc.lfnst_nz(w, h)]:
            allowed[y, x] = True
        assert not c[~allowed].any(), "LFNST levels outside the coded scan positions"
    else:
        mw, mh = (w, h) if tsf else (min(w, 32 if dct2[0] else 16), min(h, 32 if dct2[1] else 16))
        assert 1 <= nzw <= mw and 1 <= nzh <= mh, "a level window beyond the zero-out"
    assert not c[nzh:].any() and not c[:, nzw:].any(), "levels outside their window"
    if bdpcm:
        assert np.abs(np.cumsum(c.astype(np.int64), axis=0 if vert else 1)).max() <= min(lim, (1 << pic.rbits) - 1)
    return c, int(nzw), int(nzh)


def _levels(rng, pic, w, h, qp, dep, tsf, bdpcm=0, vert=0, lfnst=False, dct2=(True, True), cu=None, c_idx=0):
    """(levels (h, w) int32, nzw, nzh) inside the domain.  A picture drawn with levels= asks its hook first (None: the draw below)."""
    lw, lh = w.bit_length() - 1, h.bit_length() - 1
    lim = _level_limit(pic, lw, lh, qp, dep, tsf)
    assert lim >= 1
    hook = getattr(pic, "levels_hook", None)
    if hook is not None:
        drawn = hook(rng, pic, w, h, qp, dep, tsf, bdpcm=bdpcm, vert=vert, lfnst=lfnst, dct2=dct2, lim=lim, cu=cu, c_idx=c_idx)
        if drawn is not None:
            return _hooked_levels(pic, drawn, w, h, lim, tsf, bdpcm, vert, lfnst, dct2)
    if lfnst:
        c = np.zeros((h, w), np.int32)
        for (x, y) in DIAG4[:itc.lfnst_nz(w, h)]:
            c[y, x] = int(rng.integers(-40, 41)) if rng.random() < 0.7 else 0
        if not c.any():
            c[0, 0] = 3
        nzw, nzh = int(np.nonzero(c.any(axis=0))[0].max()) + 1, int(np.nonzero(c.any(axis=1))[0].max()) + 1
    else:
        mw, mh = (w, h) if tsf else (min(w, 32 if dct2[0] else 16), min(h, 32 if dct2[1] else 16))
        full = rng.random() < 0.2
        nzw, nzh = (mw, mh) if full else (int(rng.integers(1, mw + 1)), int(rng.integers(1, mh + 1)))
        c = lc.windowed_block(rng, w, h, nzw, nzh, None if rng.random() < 0.8 else int(rng.integers(3, 15)))
    c = np.clip(c, -lim, lim).astype(np.int32)
    if bdpcm:
        while True:
            acc = np.cumsum(c.astype(np.int64), axis=0 if vert else 1)
            if np.abs(acc).max() <= min(lim, (1 << pic.rbits) - 1):
                break
            c = (c // 2).astype(np.int32)
    if not c.any():
        c[0, 0] = 1
    assert np.abs(c).max() <= lim and c.any()
    return c, nzw, nzh


def _tb(c_idx, x0, y0, w, h, has, tsf=0, levels=None, nzw=0, nzh=0):
    return dict(c_idx=c_idx, x0=x0, y0=y0, w=w, h=h, has=int(has), ts=int(tsf), levels=levels, nzw=nzw, nzh=nzh)


def _new_cu(x, y, w, h, pred_mode, tree=0):
    return dict(x0=x, y0=y, w=w, h=h, pred_mode=pred_mode, tree_type=tree, mode_y=0, mode_c=0, ref_idx=0, mip_flag=0, mip_mode=0, mip_transposed=0,
                mip_chroma_direct=0, isp_type=0, num_isp=1, bdpcm=[0, 0, 0], lfnst_idx=0, apply_lfnst=[0, 0, 0], mts_idx=0, sbt_flag=0,
                sbt_horizontal=0, sbt_pos=0, coded_flag=1, ciip_flag=0, qp=[0, 0, 0, 0], tus=[])


def _draw_qp(rng, pic):
    off = 6 * (pic.bd - 8)
    hi = min(63 + off, MAX_TB_QP, getattr(pic, "qp_max", MAX_TB_QP))
    lo = 0 if rng.random() < 0.15 else 12
    return [int(rng.integers(lo, hi + 1)) - off] + [int(rng.integers(lo, hi + 1)) for _ in range(3)]


def _chroma_tbs(rng, pic, cu, tu, x0, y0, w, h, ts_ok, sl):
    """The two chroma blocks of a transform unit (x0, y0, w, h in luma samples): coded flags, joint Cb-Cr, transform skip, levels."""
    t = pic.tools
    cw, ch = w >> pic.hs, h >> pic.vs
    coded = [int(rng.random() < t["coded"]), int(rng.random() < t["coded"])]
    bd_c = cu["bdpcm"][1]
    tu["joint"] = int(not bd_c and any(coded) and rng.random() < t["joint"])
    tu["coded"][1], tu["coded"][2] = coded
    only = (1 if coded[0] else 2) if tu["joint"] else 0
    tsf_tu = bd_c or (ts_ok and 2 <= cw <= 32 and 2 <= ch <= 32 and cw * ch >= 8 and rng.random() < t["ts"])
    out = []
    for c in (1, 2):
        has = coded[c - 1] and (not only or c == only)
        if not has:
            out.append(_tb(c, x0, y0, cw, ch, 0))
            continue
        tsf = int(bool(tsf_tu))
        lf = bool(cu["apply_lfnst"][c]) and not tsf
        qp = tb_qp(pic, cu, tu, c, tsf)
        lv, nzw, nzh = _levels(rng, pic, cw, ch, qp, sl[0], tsf, bd_c, cu["mode_c"] == 50, lf, cu=cu, c_idx=c)
        out.append(_tb(c, x0, y0, cw, ch, 1, tsf, lv, nzw, nzh))
    return out


def _hooked_modes(pic, cu, forced, ctb):
    """What a modes= hook asks of an intra unit whose tools are drawn: prediction modes only, where the drawn tools leave them free."""
    for k, v in (forced or {}).items():
        if k == "mode_y":
            assert cu["tree_type"] != 2 and not cu["mip_flag"] and not cu["bdpcm"][0] and 0 <= v <= 66 and (v != 0 or not cu["ref_idx"])
        elif k == "mode_c":
            assert pic.idc and cu["tree_type"] != 1 and not cu["bdpcm"][1] and (0 <= v <= 66 or 81 <= v <= 83)
            cu["mip_chroma_direct"] = 0
        elif k == "ref_idx":
            assert 0 <= v <= 2 and (v == 0 or (cu["tree_type"] != 2 and not cu["isp_type"] and not cu["mip_flag"] and not cu["bdpcm"][0] and
                                               forced.get("mode_y", cu["mode_y"]) != 0 and (cu["y0"] & (ctb - 1))))
        elif k == "mip_mode":
            size_id = 0 if (cu["w"] == 4 and cu["h"] == 4) else 1 if (cu["w"] == 4 or cu["h"] == 4 or (cu["w"] == 8 and cu["h"] == 8)) else 2
            assert cu["mip_flag"] and 0 <= v < (16, 8, 6)[size_id]
        else:
            assert k == "mip_transposed" and cu["mip_flag"] and v in (0, 1), k
        cu[k] = int(v)


def _intra_cu(rng, pic, x, y, w, h, tree, sl):
    """An intra coding unit as a parser could leave it: single tree (luma + chroma), dual-tree luma or dual-tree chroma."""
    t = pic.tools
    ctb = 1 << pic.ctb_log2
    cu = _new_cu(x, y, w, h, 1, tree)
    cu["qp"] = _draw_qp(rng, pic)
    chroma = pic.idc != 0 and tree != 1
    cw, ch = w >> pic.hs, h >> pic.vs
    if tree != 2:
        mode = int(rng.integers(0, 67))
        isp = w * h > 16 and rng.random() < t["isp"]
        mip = not isp and rng.random() < t["mip"]
        if mip:
            size_id = 0 if (w == 4 and h == 4) else 1 if (w == 4 or h == 4 or (w == 8 and h == 8)) else 2
            cu["mip_flag"], cu["mip_mode"], cu["mip_transposed"] = 1, int(rng.integers(0, (16, 8, 6)[size_id])), int(rng.integers(0, 2))
            mode = 0
        if not isp and not mip and mode != 0 and (y & (ctb - 1)) and rng.random() < t["ref_line"]:
            cu["ref_idx"] = int(rng.integers(1, 3))
        if not isp and not mip and not cu["ref_idx"] and w <= 32 and h <= 32 and rng.random() < t["bdpcm"]:
            cu["bdpcm"][0], mode = 1, int(rng.choice([18, 50]))
        if w != h and not mip and not cu["bdpcm"][0]:
            mode = 2 + pic.angular % 65                                       # non-square units walk through every angular mode
            pic.angular += 1
        cu["mode_y"] = mode
        parts = [(x + dx, y + dy, min(w, 64), min(h, 64)) for dy in range(0, h, 64) for dx in range(0, w, 64)]
        if isp:
            n = 2 if (w, h) in ((4, 8), (8, 4)) else 4
            ver = (w >= n and rng.random() < 0.5) or h < n
            cu["isp_type"], cu["num_isp"] = (2 if ver else 1), n
            parts = [(x + i * (w // n), y, w // n, h) for i in range(n)] if ver else [(x, y + i * (h // n), w, h // n) for i in range(n)]
        small = min(p[2] for p in parts) >= 4 and min(p[3] for p in parts) >= 4
        if not cu["bdpcm"][0] and small and (not mip or (w >= 16 and h >= 16)) and rng.random() < t["lfnst"]:
            cu["lfnst_idx"], cu["apply_lfnst"][0] = int(rng.integers(1, 3)), 1
        ts_y = cu["bdpcm"][0] or (not isp and not cu["lfnst_idx"] and w <= 32 and h <= 32 and rng.random() < t["ts"])
        if pic.explicit_mts_intra and pic.mts_enabled and not isp and not cu["lfnst_idx"] and not ts_y and w <= 32 and h <= 32 and rng.random() < t["mts"]:
            cu["mts_idx"] = int(rng.integers(1, 5))
    else:
        parts = [(x, y, w, h)]
    if chroma:
        r = rng.random()
        if r < t["cclm"]:
            cu["mode_c"] = int(rng.integers(81, 84))
        elif r < t["cclm"] + 0.25 and tree != 2:
            cu["mode_c"] = cu["mode_y"]                                       # the derived mode
            cu["mip_chroma_direct"] = int(cu["mip_flag"] and pic.idc == 3)
        else:
            cu["mode_c"] = int(rng.choice([0, 1, 18, 50, int(rng.integers(2, 67))]))
        if cw <= 32 and ch <= 32 and cw * ch >= 8 and min(cw, ch) >= 2 and rng.random() < t["bdpcm"]:
            cu["bdpcm"][1] = cu["bdpcm"][2] = 1
            cu["mode_c"], cu["mip_chroma_direct"] = int(rng.choice([18, 50])), 0
        if tree == 2 and not cu["bdpcm"][1] and cw >= 4 and ch >= 4 and rng.random() < t["lfnst"]:
            cu["lfnst_idx"], cu["apply_lfnst"][1], cu["apply_lfnst"][2] = int(rng.integers(1, 3)), 1, 1
    if getattr(pic, "modes_hook", None) is not None:
        _hooked_modes(pic, cu, pic.modes_hook(pic, cu), ctb)
    for i, (px_, py, pw, ph) in enumerate(parts):
        tu = dict(x0=px_, y0=py, w=pw, h=ph, coded=[0, 0, 0], joint=0, tbs=[])
        if tree != 2:
            has = rng.random() < t["coded"]
            tu["coded"][0] = int(has)
            if has:
                tsf = int(bool(ts_y))
                qp = tb_qp(pic, cu, tu, 0, tsf)
                lv, nzw, nzh = _levels(rng, pic, pw, ph, qp, sl[0], tsf, cu["bdpcm"][0], cu["mode_y"] == 50, bool(cu["apply_lfnst"][0]) and not tsf,
                                       tr_kinds(pic, cu, 0, pw, ph), cu=cu)
                tu["tbs"].append(_tb(0, px_, py, pw, ph, 1, tsf, lv, nzw, nzh))
            else:
                tu["tbs"].append(_tb(0, px_, py, pw, ph, 0))
        if chroma and (cu["isp_type"] == 0 or i == len(parts) - 1):
            r = (x, y, w, h) if cu["isp_type"] else (px_, py, pw, ph)
            tu["tbs"] += _chroma_tbs(rng, pic, cu, tu, *r, ts_ok=True, sl=sl)
        cu["tus"].append(tu)
    return cu


def _inter_cu(rng, pic, x, y, w, h, sl, coded=None):
    """An inter coding unit: uncoded (drawn, or coded=False), or transform units per 64x64 tile, or the two transform units of SBT with one
    of them coded."""
    t = pic.tools
    cu = _new_cu(x, y, w, h, 0)
    cu["qp"] = _draw_qp(rng, pic)
    if (rng.random() >= t["cu_coded"]) if coded is None else not coded:
        cu["coded_flag"] = 0
        return cu
    tiles = [(x + dx, y + dy, min(w, 64), min(h, 64)) for dy in range(0, h, 64) for dx in range(0, w, 64)]
    coded_part = None
    if w <= 64 and h <= 64 and max(w, h) >= 8 and rng.random() < t["sbt"]:
        hor = (h >= 8 and rng.random() < 0.5) or w < 8
        quad = (h if hor else w) >= 16 and rng.random() < 0.4
        pos = int(rng.integers(0, 2))
        cu["sbt_flag"], cu["sbt_horizontal"], cu["sbt_pos"] = 1, int(hor), pos
        full = h if hor else w
        a = full // 4 if quad else full // 2
        first = a if not pos else full - a                                   # the coded part lies first (pos 0) or last (pos 1)
        sizes = (first, full - first)
        tiles = [(x, y, w, sizes[0]), (x, y + sizes[0], w, sizes[1])] if hor else [(x, y, sizes[0], h), (x + sizes[0], y, sizes[1], h)]
        coded_part = pos
    elif pic.explicit_mts_inter and pic.mts_enabled and w <= 32 and h <= 32 and rng.random() < t["mts"]:
        cu["mts_idx"] = int(rng.integers(1, 5))
    ts_cu = not cu["sbt_flag"] and not cu["mts_idx"] and w <= 32 and h <= 32 and rng.random() < t["ts"]
    for i, (px_, py, pw, ph) in enumerate(tiles):
        tu = dict(x0=px_, y0=py, w=pw, h=ph, coded=[0, 0, 0], joint=0, tbs=[])
        live = coded_part is None or i == coded_part
        has = live and rng.random() < t["coded"]
        tu["coded"][0] = int(has)
        if has:
            tsf = int(bool(ts_cu))
            qp = tb_qp(pic, cu, tu, 0, tsf)
            lv, nzw, nzh = _levels(rng, pic, pw, ph, qp, sl[0], tsf, dct2=tr_kinds(pic, cu, 0, pw, ph), cu=cu)
            tu["tbs"].append(_tb(0, px_, py, pw, ph, 1, tsf, lv, nzw, nzh))
        else:
            tu["tbs"].append(_tb(0, px_, py, pw, ph, 0))
        if pic.idc:
            if live:
                tu["tbs"] += _chroma_tbs(rng, pic, cu, tu, px_, py, pw, ph, ts_ok=not cu["sbt_flag"], sl=sl)
            else:
                tu["tbs"] += [_tb(c, px_, py, pw >> pic.hs, ph >> pic.vs, 0) for c in (1, 2)]
        cu["tus"].append(tu)
    return cu


def draw(name, seed, bd, idc, ctb_log2, size, intra=1.0, slices=((0, 0),), lmcs=False, tiles=False, wpp=0, collocated=0, rbits=15, dual=False,
         big_inter=False, inter_ctu=0.0, min_cu=8, mts=True, explicit_mts=False, min_qp_prime_ts=0, joint_sign=0, tools=None, angular=0,
         content=None, levels=None, units=None, modes=None, model=None, qp_max=MAX_TB_QP, partition=None):
    """The unit-level description of one picture.  The hooks default to what is drawn here (every listed and swept picture: none set):
      content(rng, pic, dims) -> the three starting planes, dims = [(h, w)] * 3 (4:0:0: two unused planes of half size);
      levels(rng, pic, w, h, qp, dep, ts, bdpcm=, vert=, lfnst=, dct2=, lim=, cu=, c_idx=) -> (levels, nzw, nzh) of one coded block, or None
          for the draw of _levels(); dct2 is tr_kinds()'s pair, lim the dequant limit of the block; the result is held to the domain;
      units(pic, rs, x, y, w, h) -> "intra" / "inter" / "skip" (an inter unit without residual) for one leaf of the partition, or None;
      modes(pic, cu) -> {mode_y, mode_c, ref_idx, mip_mode, mip_transposed} to force on an intra unit whose tools are drawn, or None;
      partition(pic, rs) -> the leaves [(x, y, w, h)] of a single-tree CTU in coding order (power-of-two sides, tiling the CTU's part of the
          picture), or None for the drawn partition;
      model(bd) -> the LMCS model of a picture with lmcs=True; qp_max: the largest QP _draw_qp draws."""
    rng = np.random.default_rng(seed)
    W, H = size
    hs, vs = FMT[idc]
    ctb = 1 << ctb_log2
    ncx, ncy = (W + ctb - 1) // ctb, (H + ctb - 1) // ctb
    n_ctb = ncx * ncy
    pic = SimpleNamespace(name=name, bd=bd, idc=idc, hs=hs, vs=vs, ctb_log2=ctb_log2, width=W, height=H, ncx=ncx, ncy=ncy, rbits=rbits, wpp=wpp,
                          collocated=collocated, mts_enabled=int(mts), explicit_mts_intra=int(mts and explicit_mts), explicit_mts_inter=int(mts and explicit_mts),
                          min_qp_prime_ts=min_qp_prime_ts, joint_sign=joint_sign, chroma_scale_flag=int(lmcs and idc != 0), slices=[tuple(s) for s in slices],
                          tools=dict(DEFAULT_TOOLS, **(tools or {})), size_y=min(ctb, 64), isz=1 if bd == 8 else 2, angular=angular,
                          levels_hook=levels, modes_hook=modes, qp_max=qp_max)
    n_sl = len(pic.slices)
    cuts = sorted(rng.choice(np.arange(1, n_ctb), size=n_sl - 1, replace=False).tolist()) if n_sl > 1 else []
    pic.slice_idx = np.searchsorted(cuts, np.arange(n_ctb), side="right").astype(np.int16)
    if tiles and ncx > 2 and ncy > 1:
        cx, cy = int(rng.integers(1, ncx)), int(rng.integers(1, ncy))
        pic.col_bd = np.array([0 if x < cx else cx for x in range(ncx)] + [ncx], np.int16)
        pic.row_bd = np.array([0 if y < cy else cy for y in range(ncy)] + [ncy], np.int16)
    else:
        pic.col_bd, pic.row_bd = np.array([0] * ncx + [ncx], np.int16), np.array([0] * ncy + [ncy], np.int16)
    pic.model = (model(bd) if model is not None else recon_cases.ReconWork.lmcs_model(rng, bd)) if lmcs else abi.LmcsModel()
    dims = [(H, W)] + [((H >> vs, W >> hs) if idc else (H >> 1, W >> 1))] * 2
    if content is not None:
        pic.planes = [np.ascontiguousarray(p, px(bd)) for p in content(rng, pic, dims)]
        assert [p.shape for p in pic.planes] == dims and all(int(p.max()) < (1 << bd) for p in pic.planes)
    elif lmcs:
        # an own DC level per 32x32 unit under the smooth content: neighbouring 64x64 units then fall into different bins of the model
        luma = bc.smooth_picture(rng, H, W, bd).astype(np.int64) // 4 + np.kron(rng.integers(0, 3 << (bd - 2), size=((H + 31) // 32, (W + 31) // 32)),
                                                                                 np.ones((32, 32), np.int64))[:H, :W]
        planes = [np.clip(luma, 0, (1 << bd) - 1).astype(px(bd))]
    else:
        planes = [bc.smooth_picture(rng, H, W, bd)]
    if content is None:
        pic.planes = planes + [bc.smooth_picture(rng, dh, dw, bd) for (dh, dw) in dims[1:]]
    pic.ctus = []
    whole_inter = rng.random(n_ctb) < inter_ctu
    for rs in range(n_ctb):
        rx, ry = rs % ncx, rs // ncx
        sl = pic.slices[int(pic.slice_idx[rs])]
        leaves, cus = [], []
        directed = partition(pic, rs) if partition is not None and not dual else None
        if directed is None:
            _split(rng, rx * ctb, ry * ctb, ctb, ctb, W, H, min_cu, leaves, big_inter)
        else:
            leaves = [tuple(v) for v in directed]
            cover = np.zeros((min(ctb, H - ry * ctb), min(ctb, W - rx * ctb)), np.int32)
            for (x, y, w, h) in leaves:
                assert w & (w - 1) == 0 and h & (h - 1) == 0 and min(w, h) >= 4 and x % min(w, 8) == 0 and y % min(h, 8) == 0
                cover[y - ry * ctb:y - ry * ctb + h, x - rx * ctb:x - rx * ctb + w] += 1
            assert (cover == 1).all() and sum(w * h for (_x, _y, w, h) in leaves) == cover.size, "a directed partition does not tile its CTU"
        if dual:
            for (x, y, w, h) in leaves:
                cus.append(_intra_cu(rng, pic, x, y, w, h, 1, sl))
            leaves_c = []
            _split(rng, rx * ctb, ry * ctb, ctb, ctb, W, H, 8, leaves_c, False)
            for (x, y, w, h) in leaves_c:
                cus.append(_intra_cu(rng, pic, x, y, w, h, 2, sl))
        else:
            for (x, y, w, h) in leaves:
                # the standard has no intra chroma block under 4 samples wide or 16 samples (the reference's predictors write 4 columns
                # there); units too small for that are inter units here, down to 4x4, which the standard does not have but the reference's
                # and the record passes' residual paths do: their 2x2 chroma blocks are the ones chroma residual scaling leaves alone
                small_c = idc != 0 and ((w >> hs) < 4 or (w >> hs) * (h >> vs) < 16)
                forced = units(pic, rs, x, y, w, h) if units is not None else None
                if forced is None:
                    is_intra = not whole_inter[rs] and not small_c and w <= 64 and h <= 64 and rng.random() < intra
                else:
                    is_intra = forced == "intra"
                    assert forced in ("intra", "inter", "skip") and not (is_intra and (small_c or w > 64 or h > 64)), forced
                cus.append(_intra_cu(rng, pic, x, y, w, h, 0, sl) if is_intra else
                           _inter_cu(rng, pic, x, y, w, h, sl, coded=False if forced == "skip" else None))
        pic.ctus.append(cus)
    return pic


_pictures = {}


def picture_names():
    return list(_LISTED)


def picture(name):
    """A listed picture; made once, nobody writes to it."""
    if name not in _pictures:
        _pictures[name] = draw(name, SEED + list(_LISTED).index(name), **_LISTED[name])
    return _pictures[name]


def sweep_picture(k, salt=0):
    """Freshly drawn picture k of a sweep: free size up to 264x136, free format, CTU, flags and unit mix."""
    rng = np.random.default_rng([SEED, 0x5EE9, salt, k])
    ctb_log2 = int(rng.integers(5, 8))
    kw = dict(bd=int(rng.choice([8, 10, 12])), idc=int(rng.integers(0, 4)), ctb_log2=ctb_log2,
              size=(8 * int(rng.integers(5, 34)), 8 * int(rng.integers(5, 18))), intra=float(rng.choice([0.3, 0.6, 1.0])),
              slices=[(int(rng.integers(0, 2)), int(rng.random() < 0.75)) for _ in range(int(rng.integers(1, 4)))], lmcs=bool(rng.random() < 0.8),
              tiles=bool(rng.random() < 0.4), wpp=int(rng.integers(0, 2)), collocated=int(rng.integers(0, 2)), dual=bool(rng.random() < 0.15),
              big_inter=bool(rng.random() < 0.5), inter_ctu=float(rng.choice([0.0, 0.4, 0.7])), min_cu=int(rng.choice([4, 8, 8])),
              angular=int(rng.integers(0, 65)), mts=bool(rng.random() < 0.8), explicit_mts=bool(rng.random() < 0.5), min_qp_prime_ts=int(rng.integers(0, 3)), joint_sign=int(rng.integers(0, 2)))
    kw["rbits"] = 18 if kw["bd"] == 12 and rng.random() < 0.4 else 15
    n_ctb = -(-kw["size"][0] >> ctb_log2) * -(-kw["size"][1] >> ctb_log2)
    kw["slices"] = kw["slices"][:max(1, min(len(kw["slices"]), n_ctb))]
    return draw(f"sweep{salt}/{k}", int(rng.integers(1 << 31)), **kw)


# ---------------------------------------------------------------------------------------------------------------- (a) the shim's arrays

_I = "<i4"
TB_DT = np.dtype([(n, _I) for n in ("c_idx", "x0", "y0", "w", "h", "ts", "has_coeffs", "min_x", "min_y", "max_x", "max_y", "level_off")])
TU_DT = np.dtype([("x0", _I), ("y0", _I), ("w", _I), ("h", _I), ("coded_flag", _I, 3), ("joint", _I), ("first_tb", _I), ("n_tbs", _I)])
CU_DT = np.dtype([("x0", _I), ("y0", _I), ("w", _I), ("h", _I), ("pred_mode", _I), ("tree_type", _I), ("mode_y", _I), ("mode_c", _I), ("ref_idx", _I),
                  ("mip_flag", _I), ("mip_mode", _I), ("mip_transposed", _I), ("mip_chroma_direct", _I), ("isp_type", _I), ("num_isp", _I), ("bdpcm", _I, 3),
                  ("lfnst_idx", _I), ("apply_lfnst", _I, 3), ("mts_idx", _I), ("sbt_flag", _I), ("sbt_horizontal", _I), ("sbt_pos", _I), ("coded_flag", _I),
                  ("ciip_flag", _I), ("qp", _I, 4), ("first_tu", _I), ("n_tus", _I)])


class MirReconPic(ctypes.Structure):
    """Mirror of the shim's MirReconPic."""
    _fields_ = [("plane", ctypes.c_uint64 * 3), ("slice_idx", ctypes.c_uint64), ("col_bd", ctypes.c_uint64), ("row_bd", ctypes.c_uint64),
                ("slice_dep_quant", ctypes.c_uint64), ("slice_lmcs_used", ctypes.c_uint64), ("ctu_first_cu", ctypes.c_uint64), ("cus", ctypes.c_uint64),
                ("tus", ctypes.c_uint64), ("tbs", ctypes.c_uint64), ("levels", ctypes.c_uint64), ("scale_log", ctypes.c_uint64),
                ("stride", ctypes.c_int32 * 3), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bit_depth", ctypes.c_int32),
                ("chroma_format_idc", ctypes.c_int32), ("ctb_log2", ctypes.c_int32), ("wpp", ctypes.c_int32), ("collocated", ctypes.c_int32),
                ("mts_enabled", ctypes.c_int32), ("explicit_mts_intra", ctypes.c_int32), ("explicit_mts_inter", ctypes.c_int32),
                ("log2_transform_range", ctypes.c_int32), ("min_qp_prime_ts", ctypes.c_int32), ("joint_cbcr_sign", ctypes.c_int32),
                ("chroma_residual_scale", ctypes.c_int32), ("lmcs_min_bin_idx", ctypes.c_int32), ("lmcs_max_bin_idx", ctypes.c_int32),
                ("lmcs_pivot", ctypes.c_int32 * 17), ("lmcs_chroma_scale_coeff", ctypes.c_int32 * 16), ("n_slices", ctypes.c_int32),
                ("n_levels", ctypes.c_int32), ("scale_log_cap", ctypes.c_int32), ("n_scale_log", ctypes.c_int32)]


def shim_arrays(pic):
    """The flat arrays of a picture: (ctu_first_cu, cus, tus, tbs, levels).  Made once per picture."""
    if getattr(pic, "_flat", None) is not None:
        return pic._flat
    first, cus, tus, tbs, levels, n_lv = [0], [], [], [], [], 0
    for ctu in pic.ctus:
        for cu in ctu:
            first_tu = len(tus)
            for tu in cu["tus"]:
                first_tb = len(tbs)
                for b in tu["tbs"]:
                    n = b["w"] * b["h"]
                    lv = b["levels"] if b["has"] else np.zeros((b["h"], b["w"]), np.int32)
                    nz = np.nonzero(lv)
                    mn = (int(nz[1].min()), int(nz[0].min())) if len(nz[0]) else (0, 0)
                    tbs.append((b["c_idx"], b["x0"], b["y0"], b["w"], b["h"], b["ts"], b["has"], mn[0], mn[1], max(b["nzw"], 1) - 1, max(b["nzh"], 1) - 1, n_lv))
                    levels.append(lv.ravel())
                    n_lv += n
                tus.append((tu["x0"], tu["y0"], tu["w"], tu["h"], tuple(tu["coded"]), tu["joint"], first_tb, len(tu["tbs"])))
            cus.append(tuple(cu[k] if not isinstance(cu[k], list) else tuple(cu[k]) for k in CU_DT.names[:-2]) + (first_tu, len(cu["tus"])))
        first.append(len(cus))
    pic._flat = (np.array(first, np.int32), np.array(cus, CU_DT) if cus else np.zeros(0, CU_DT), np.array(tus, TU_DT) if tus else np.zeros(1, TU_DT),
                 np.array(tbs, TB_DT) if tbs else np.zeros(1, TB_DT), np.concatenate(levels).astype(np.int32) if levels else np.zeros(1, np.int32))
    return pic._flat


def bind_reference(lib):
    lib.ref_recon_picture.argtypes = [ctypes.POINTER(MirReconPic)]
    lib.ref_recon_picture.restype = ctypes.c_int
    lib.ref_recon_layout.argtypes = [ctypes.c_int]
    lib.ref_recon_layout.restype = ctypes.c_int
    assert [lib.ref_recon_layout(i) for i in range(6)] == [ctypes.sizeof(MirReconPic), CU_DT.itemsize, TU_DT.itemsize, TB_DT.itemsize,
                                                           MirReconPic.stride.offset, MirReconPic.n_slices.offset], "the shim's arrays and their mirror differ"


def mirror(pic, planes, log):
    """(MirReconPic over `planes` and the int32 [n][3] scale log, the arrays it points to: keep them while it is used)."""
    first, cus, tus, tbs, levels = shim_arrays(pic)
    dep, used = np.array([s[0] for s in pic.slices], np.int32), np.array([s[1] for s in pic.slices], np.int32)
    col, row = pic.col_bd.astype(np.uint16), pic.row_bd.astype(np.uint16)
    m = MirReconPic()
    for c in range(3):
        m.plane[c], m.stride[c] = planes[c].ctypes.data, planes[c].strides[0]
    m.slice_idx, m.col_bd, m.row_bd = pic.slice_idx.ctypes.data, col.ctypes.data, row.ctypes.data
    m.slice_dep_quant, m.slice_lmcs_used = dep.ctypes.data, used.ctypes.data
    m.ctu_first_cu, m.cus, m.tus, m.tbs, m.levels, m.scale_log = (a.ctypes.data for a in (first, cus, tus, tbs, levels, log))
    m.width, m.height, m.bit_depth, m.chroma_format_idc, m.ctb_log2 = pic.width, pic.height, pic.bd, pic.idc, pic.ctb_log2
    m.wpp, m.collocated, m.mts_enabled, m.explicit_mts_intra, m.explicit_mts_inter = pic.wpp, pic.collocated, pic.mts_enabled, pic.explicit_mts_intra, pic.explicit_mts_inter
    m.log2_transform_range, m.min_qp_prime_ts, m.joint_cbcr_sign, m.chroma_residual_scale = pic.rbits, pic.min_qp_prime_ts, pic.joint_sign, pic.chroma_scale_flag
    m.lmcs_min_bin_idx, m.lmcs_max_bin_idx = pic.model.min_bin_idx, pic.model.max_bin_idx
    for i in range(17):
        m.lmcs_pivot[i] = pic.model.pivot[i]
    for i in range(16):
        m.lmcs_chroma_scale_coeff[i] = pic.model.chroma_scale_coeff[i]
    m.n_slices, m.n_levels, m.scale_log_cap = len(pic.slices), len(levels), len(log)
    return m, (dep, used, col, row)


def scales_of(log, n):
    """The first n entries of a scale log: ({(x_vpdu, y_vpdu): chroma_scale}, units logged with two values)."""
    scales, twice = {}, []
    for x, y, s in log[:n].tolist():
        if scales.setdefault((x, y), s) != s:
            twice.append((x, y))
    return scales, twice


def run_reference(lib, pic):
    """ff_vvc_reconstruct over the picture: (return value, planes, scale log {(x_vpdu, y_vpdu): chroma_scale}, units logged with two values)."""
    bind_reference(lib)
    levels = shim_arrays(pic)[4]
    planes = [np.ascontiguousarray(p).copy() for p in pic.planes]
    log = np.zeros((4 * len(shim_arrays(pic)[3]) + 4, 3), np.int32)
    m, _keep = mirror(pic, planes, log)
    before = levels.copy()
    ret = lib.ref_recon_picture(ctypes.byref(m))
    assert np.array_equal(levels, before) and m.n_scale_log <= len(log)
    scales, twice = scales_of(log, m.n_scale_log)
    return ret, planes, scales, twice


# ---------------------------------------------------------------------------------------------------------------- (b) the project's inputs

def _tables(pic):
    """What the parser paints per 4x4 unit and derive_ilfnst_pred_mode_intra reads: IntraMipFlag, IntraPredModeY, CuPredMode (luma tree)."""
    ph, pw = (pic.height + 3) // 4, (pic.width + 3) // 4
    imf, ipm, cpm = np.zeros((ph, pw), np.uint8), np.zeros((ph, pw), np.uint8), np.zeros((ph, pw), np.uint8)
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] != 2:
                s = np.s_[cu["y0"] // 4:(cu["y0"] + cu["h"] + 3) // 4, cu["x0"] // 4:(cu["x0"] + cu["w"] + 3) // 4]
                imf[s], ipm[s], cpm[s] = cu["mip_flag"], cu["mode_y"], cu["pred_mode"]
    return imf, ipm, cpm


def wide_angle(isp, c_idx, w, h, cb_w, cb_h, mode):
    """8.4.5.2.7 as the records' pred_mode_intra needs it (the formula of the standard; dsp_ctx_shim.c restates it too)."""
    nw, nh = (w, h) if (not isp or c_idx) else (cb_w, cb_h)
    r = abs(nw.bit_length() - nh.bit_length())
    hi, lo = (8 + 2 * r, 60 - 2 * r) if r > 1 else (8, 60)
    if nw > nh and 2 <= mode < hi:
        return mode + 65
    if nh > nw and lo < mode <= 66:
        return mode - 67
    return mode


def lfnst_mode(pic, tabs, cu, b):
    """derive_ilfnst_pred_mode_intra (vvc_intra.c:34-62) from the unit description: the record's pred_mode_intra."""
    imf, ipm, cpm = tabs
    c = b["c_idx"]
    mode = cu["mode_c"] if c else cu["mode_y"]
    if c == 0 and imf[b["y0"] >> 2, b["x0"] >> 2]:
        mode = 0
    elif 81 <= mode <= 83:
        xc, yc = (b["x0"] + (b["w"] << pic.hs >> 1)) >> 2, (b["y0"] + (b["h"] << pic.vs >> 1)) >> 2
        mode = 0 if imf[yc, xc] else 1 if cpm[yc, xc] != 1 else int(ipm[yc, xc])
    return wide_angle(cu["isp_type"] != 0, c, b["w"], b["h"], cu["w"], cu["h"], mode)


def derive(pic, misread=None):
    """The project's inputs of a picture by INTEGRATION.md section 3.  `misread`: one of MISREADINGS, applied here alone."""
    assert misread is None or misread in MISREADINGS
    hs, vs, ctb_log2, ncx = pic.hs, pic.vs, pic.ctb_log2, pic.ncx
    tabs = _tables(pic)
    has_intra = [any(cu["pred_mode"] == 1 for cu in ctu) for ctu in pic.ctus]
    sy = pic.size_y
    sign = 0 if misread == "joint_sign_dropped" else pic.joint_sign

    def ctu_of(x, y):
        return (y >> ctb_log2) * ncx + (x >> ctb_log2)

    def needs_walk(cu):
        """The unit's 64x64 unit reads luma left of / above itself: does the walk write that luma?"""
        xv, yv = cu["x0"] & ~(sy - 1), cu["y0"] & ~(sy - 1)
        return (xv > 0 and has_intra[ctu_of(xv - 1, yv)]) or (yv > 0 and has_intra[ctu_of(xv, yv - 1)])

    intra, inter, skip = [], [], []           # specs of the three record passes; spec["rid"] ties a RESID command to its arena slot
    rid = [0]
    cmds, ctus = [], np.zeros(len(pic.ctus), CTU)
    kind = np.zeros(len(pic.ctus), np.int8)
    routed, walked = set(), set()
    stats = dict(keep=0, batched_scaled=0, walk_scaled=0)
    for rs, ctu in enumerate(pic.ctus):
        sl = pic.slices[int(pic.slice_idx[rs])]
        out, any_resid = [], False
        for cu in ctu:
            cur = (cu["x0"], cu["y0"], cu["w"], cu["h"])
            if not cu["coded_flag"]:
                if misread != "no_mark_for_uncoded_unit":
                    out.append(_cmd(abi.RECON_MARK, 0, *cur, *cur))
                    out.append(_cmd(abi.RECON_MARK, 1, *cur, *cur))
                continue
            is_intra = cu["pred_mode"] == 1
            for ch in range(int(cu["tree_type"] == 2), 1 + int(pic.idc != 0 and cu["tree_type"] != 1)):
                for i, tu in enumerate(cu["tus"]):
                    tr = (tu["x0"], tu["y0"], tu["w"], tu["h"])
                    # ---- predict_intra
                    if not is_intra:
                        out.append(_cmd(abi.RECON_MARK, ch, *tr, *cur))
                    elif ch == 0:
                        x0, y0, w, h = tr
                        has = True
                        if cu["isp_type"] == 2 and w < 4:
                            has = i % (4 // w) == 0
                            if misread == "isp_prediction_on_every_part":
                                has, x0 = True, cu["x0"] + ((x0 - cu["x0"]) & ~3)
                            w = 4
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
                    # ---- itransform
                    for b in tu["tbs"]:
                        c = b["c_idx"]
                        if (c > 0) != ch or not b["has"]:
                            continue
                        w, h = b["w"], b["h"]
                        lw, lh = w.bit_length() - 1, h.bit_length() - 1
                        scale = 8 if (c and sl[1] and pic.chroma_scale_flag and w * h > 4) else 0
                        jb = (1 | sign << 1 | (tu["coded"][1] ^ tu["coded"][2]) << 2) if (tu["joint"] and c) else 0
                        qp = tb_qp(pic, cu, tu, c, b["ts"])
                        x_c, y_c = b["x0"] >> (hs if c else 0), b["y0"] >> (vs if c else 0)
                        walk = is_intra or bool(scale and needs_walk(cu))
                        unit_cu = None if misread == "scale_from_block_unit" else (cu["x0"], cu["y0"])
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
                                         lfnst_mode(pic, tabs, cu, b) if lf else 0, flags, cu["mts_idx"])
                            intra.append(s)
                        else:
                            flags = ((abi.TU_MTS_ENABLED if pic.mts_enabled else 0) | (abi.TU_SBT if cu["sbt_flag"] else 0) |
                                     (abi.TU_SBT_HORIZONTAL if cu["sbt_horizontal"] else 0) | (abi.TU_SBT_POS if cu["sbt_pos"] else 0))
                            s = tc.spec(c, x_c, y_c, lw, lh, b["levels"], b["nzw"], b["nzh"], qp=qp, dep=sl[0], tu_flags=flags, mts_idx=cu["mts_idx"],
                                        joint=0 if walk else scale | jb, keep=walk, cu=unit_cu)
                            inter.append(s)
                        s["rid"] = rid[0]
                        rid[0] += 1
                        unit = (cu["x0"] // sy, cu["y0"] // sy)
                        if not walk:
                            if scale:
                                routed.add(unit)
                                stats["batched_scaled"] += 1
                            continue
                        stats["keep"] += 1
                        if scale:
                            walked.add(unit)
                            stats["walk_scaled"] += not is_intra
                        any_resid = True
                        org = (b["x0"], b["y0"], cu["w"], cu["h"]) if misread == "scale_from_block_unit" else cur
                        out.append(_cmd(abi.RECON_RESID, c, b["x0"], b["y0"], w, h, *org, resid=s["rid"], joint=scale))
                        if jb:
                            out.append(_cmd(abi.RECON_RESID, 3 - c, b["x0"], b["y0"], w, h, *org, resid=s["rid"], joint=scale | jb))
        if has_intra[rs] or any_resid:
            ctus[rs]["first_cmd"], ctus[rs]["n_cmd"] = len(cmds), len(out)
            cmds += out
            kind[rs] = 2 if has_intra[rs] else 1
    for rs in np.nonzero(kind == 1)[0]:
        rx, ry = rs % ncx, rs // ncx
        ctus[rs]["flags"] = (abi.RECON_CTU_LIGHT | (abi.RECON_CTU_LUMA_LEFT if rx and kind[rs - 1] == 2 else 0) |
                             (abi.RECON_CTU_LUMA_UP if ry and kind[rs - ncx] == 2 else 0))
    d = SimpleNamespace(pic=pic, ctus=ctus, kind=kind, routed=sorted(routed), walked=sorted(walked), stats=stats)
    d.cmds = np.array(cmds, CMD) if cmds else np.zeros(0, CMD)
    d.order = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
    d.intra, d.class_first = itc.group_by_class(intra)
    d.inter, d.bin_first = tc.group(inter)
    d.skip, d.ts_first = ts.group(skip)
    d.specs = d.intra + d.inter + d.skip
    d.offs, d.arena_len = tc.arena_offsets(d.specs)
    d.off_of = {s["rid"]: o for s, o in zip(d.specs, d.offs)}
    d.tpic = tc.Picture(pic.planes, pic.bd, hs, vs, sy, ctb_log2, pic.model if pic.chroma_scale_flag else None)
    return d


def start_arena(d, lv=None):
    """Sentinels everywhere, the int32 levels of the blocks that are not packed in their slots.  lv: the side records of the three passes,
    concatenated in d.specs order."""
    return tc.start_arena(d.specs, d.offs, d.arena_len, lv)


def bound_cmds(d, base):
    """The command array with the RESID commands' slots turned into addresses at `base` (int32 arena)."""
    c = d.cmds.copy()
    is_res = c["kind"] == abi.RECON_RESID
    c["resid"][is_res] = [base + 4 * d.off_of[int(r)] for r in c["resid"][is_res]]
    return c


def scale_frame(pic, luma_ptr, luma_stride, scale_ptr, model_ptr, slice_ptr, col_ptr, row_ptr):
    """The vvc355_lmcs_scale_frame of the picture, on its own slice and tile maps."""
    f = abi.LmcsScaleFrame()
    f.luma, f.scale, f.model, f.luma_stride = luma_ptr, scale_ptr, model_ptr, luma_stride
    f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = slice_ptr, col_ptr, row_ptr
    f.width, f.height, f.ctb_width, f.ctb_log2, f.size_y = pic.width, pic.height, pic.ncx, pic.ctb_log2, pic.size_y
    return f


def recon_frame(pic, d, planes, strides, cmds_ptr, ctus_ptr, order_ptr, state_ptr, slice_ptr, col_ptr, row_ptr, model_ptr, n_work=None):
    f = abi.ReconFrame()
    for c in range(3):
        f.plane[c], f.stride[c] = planes[c], strides[c]
    f.cmds, f.ctus, f.order, f.state = cmds_ptr, ctus_ptr, order_ptr, state_ptr
    f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = slice_ptr, col_ptr, row_ptr
    f.width, f.height, f.ctb_width, f.ctb_height, f.n_work = pic.width, pic.height, pic.ncx, pic.ncy, len(d.order) if n_work is None else n_work
    f.ctb_log2, f.hs, f.vs, f.wpp, f.collocated = pic.ctb_log2, pic.hs, pic.vs, pic.wpp, pic.collocated
    f.lmcs_model = model_ptr
    return f


# ---------------------------------------------------------------------------------------------------------------- well-formed lists

def _waits_for(ctus, ncx, rs):
    import picture_cases
    return picture_cases.waits_for(ctus, ncx, rs)


def order_defect(ctus, ncx, ncy, order):
    """vvc355_recon_order_check's rules restated (include/vvc_mi355.h): None, or what is wrong first."""
    n = ncx * ncy
    seen = set()
    for rs in (int(v) for v in order):
        if not 0 <= rs < n:
            return f"index {rs} outside the grid"
        if not ctus[rs]["n_cmd"]:
            return f"CTU {rs} has no commands"
        if rs in seen:
            return f"CTU {rs} listed twice"
        ahead = [dep for dep in _waits_for(ctus, ncx, rs) if dep not in seen]
        if ahead:
            return f"CTU {rs} ahead of CTU {ahead[0]} it waits for"
        seen.add(rs)
    missing = [rs for rs in range(n) if ctus[rs]["n_cmd"] and rs not in seen]
    return f"CTU {missing[0]} with commands not listed" if missing else None


def well_formed(pic, d):
    """What a command list must satisfy before the device pass may see it: None, or the first defect."""
    bad = order_defect(d.ctus, pic.ncx, pic.ncy, d.order)
    if bad:
        return bad
    ctb = 1 << pic.ctb_log2
    ends = 0
    for rs in range(pic.ncx * pic.ncy):
        first, n, flags = (int(d.ctus[rs][k]) for k in ("first_cmd", "n_cmd", "flags"))
        if not n:
            continue
        if first != ends:
            return f"CTU {rs}: commands not contiguous"
        ends = first + n
        for c in d.cmds[first:first + n]:
            x0, y0, w, h, kind, c_idx = (int(c[k]) for k in ("x0", "y0", "w", "h", "kind", "c_idx"))
            lw, lh = (w << (pic.hs if c_idx else 0), h << (pic.vs if c_idx else 0)) if kind == abi.RECON_RESID else (w, h)
            if kind not in (abi.RECON_MARK, abi.RECON_PRED, abi.RECON_CCLM, abi.RECON_RESID):
                return f"CTU {rs}: command kind {kind}"
            if x0 < 0 or y0 < 0 or w <= 0 or h <= 0 or x0 + lw > pic.width or y0 + lh > pic.height:
                return f"CTU {rs}: a block outside the picture"
            if (x0 // ctb, y0 // ctb) != (rs % pic.ncx, rs // pic.ncx) or (x0 + lw - 1) // ctb != rs % pic.ncx or (y0 + lh - 1) // ctb != rs // pic.ncx:
                return f"CTU {rs}: a block outside its CTU"
            if (flags & abi.RECON_CTU_LIGHT) and (kind in (abi.RECON_PRED, abi.RECON_CCLM) or (kind == abi.RECON_RESID and c_idx == 0)):
                return f"LIGHT CTU {rs} touches luma or predicts"
            if kind == abi.RECON_RESID and (int(c["resid"]) not in d.off_of or ((c["joint"] & 8) and d.tpic.model is None)):
                return f"CTU {rs}: a RESID without a residual slot or a scaled one without a model"
    return None if ends == len(d.cmds) else "commands beyond the last CTU's"


# ---------------------------------------------------------------------------------------------------------------- the oracle side

def bind_oracle(orc):
    itc.bind_oracle(orc)
    tc.bind_oracle(orc)
    orc.orc_recon_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.ReconFrame)]
    orc.orc_recon_frame_pass.restype = None


def oracle_side(orc, d, scale_table=None):
    """The derived inputs through the oracle's pieces in INTEGRATION.md's order: (planes, scale table or None, arena).  scale_table: a table
    to scale the routed blocks with in place of the one orc_lmcs_vpdu_scale_pass gives (a sensitivity check of ref_picture_cases)."""
    bind_oracle(orc)
    pic, tp = d.pic, d.tpic
    bd, isz = pic.bd, pic.isz
    planes = [np.ascontiguousarray(p).copy() for p in pic.planes]
    arena = start_arena(d)
    n_i = len(d.intra)
    for s, off in zip(d.intra, d.offs[:n_i]):                                  # intra_tb
        arena[off:off + s["c"].size] = itc.oracle_block(orc, s, bd, pic.rbits).ravel()
    table = None
    rest = list(zip(d.specs[n_i:], d.offs[n_i:]))
    for ch in (0, 1):                                                          # inter_tb / ts_tb (1), the scale table, inter_tb / ts_tb (2)
        if ch == 1 and tp.model is not None:
            table = np.zeros(tp.ux * tp.uy, np.int16)
            f = scale_frame(pic, planes[0].ctypes.data, pic.width * isz, table.ctypes.data, ctypes.addressof(pic.model), pic.slice_idx.ctypes.data,
                            pic.col_bd.ctypes.data, pic.row_bd.ctypes.data)
            orc.orc_lmcs_vpdu_scale_pass(bd, ctypes.byref(f))
            if scale_table is not None:
                table[:] = np.asarray(scale_table, np.int16).ravel()
        for s, off in rest:
            if (s["c_idx"] > 0) != ch:
                continue
            res = ts.residual_of(orc, s, bd, pic.rbits)
            w, h, c = 1 << s["lw"], 1 << s["lh"], s["c_idx"]
            if s["keep"]:
                arena[off:off + w * h] = res.ravel()
                continue
            for (plane, joint) in [(c, s["joint"] & 8)] + ([(3 - c, s["joint"])] if s["joint"] & 1 else []):
                pw = planes[plane].shape[1]
                dst = planes[plane].ctypes.data + (s["y0"] * pw + s["x0"]) * isz
                if joint & 8:
                    ux, uy = tp.unit_of(s, "cu")
                    j = abi.LmcsResidJob()
                    j.dst, j.dst_stride, j.resid, j.w, j.h = dst, pw * isz, res.ctypes.data, w, h
                    j.luma, j.joint = table.ctypes.data + (uy * tp.ux + ux) * 2, joint | 16
                    orc.orc_lmcs_chroma_resid_block(bd, ctypes.byref(j), ctypes.byref(pic.model))
                elif joint & 1:
                    orc.orc_add_residual_joint(bd, dst, res.ctypes.data, w, h, pw * isz, -1 if joint & 2 else 1, (joint >> 2) & 1)
                else:
                    orc.orc_add_residual(bd, dst, res.ctypes.data, w, h, pw * isz)
    if len(d.order):                                                           # recon_frame_pass
        cmds = bound_cmds(d, arena.ctypes.data)
        f = recon_frame(pic, d, [p.ctypes.data for p in planes], [p.strides[0] for p in planes], cmds.ctypes.data, d.ctus.ctypes.data, d.order.ctypes.data, 0,
                        pic.slice_idx.ctypes.data, pic.col_bd.ctypes.data, pic.row_bd.ctypes.data, ctypes.addressof(pic.model))
        orc.orc_recon_frame_pass(bd, ctypes.byref(f))
    return planes, table, arena


# ---------------------------------------------------------------------------------------------------------------- digests

def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def inputs_digest(pic):
    first, cus, tus, tbs, levels = shim_arrays(pic)
    m = pic.model
    head = [pic.bd, pic.idc, pic.ctb_log2, pic.width, pic.height, pic.rbits, pic.wpp, pic.collocated, pic.mts_enabled, pic.explicit_mts_intra,
            pic.explicit_mts_inter, pic.min_qp_prime_ts, pic.joint_sign, pic.chroma_scale_flag, m.min_bin_idx, m.max_bin_idx] + list(m.pivot) + \
        list(m.chroma_scale_coeff) + [v for s in pic.slices for v in s]
    return sha(np.array(head, np.int64), pic.slice_idx, pic.col_bd, pic.row_bd, first, cus.view(np.int32), tus.view(np.int32), tbs.view(np.int32), levels, *pic.planes)


def scale_digest(d, table):
    """The scale table reduced to the units whose blocks the host routes to the TB passes (all of them units the reference asked for)."""
    t = np.zeros(0, np.int16) if table is None else np.asarray(table).reshape(d.tpic.uy, d.tpic.ux)
    return sha(np.array([(ux, uy, int(t[uy, ux])) for (ux, uy) in d.routed], np.int32).reshape(-1, 3))


def digests(pic, d, planes, table):
    n = 3 if pic.idc else 1
    out = {"inputs": inputs_digest(pic)}
    out.update({f"p{c}": sha(planes[c]) for c in range(n)})
    out["scale"] = scale_digest(d, table)
    return out


def reference_digests(lib, name):
    """One picture's record of tests/golden/ref_recon.json from the reference: planes as ff_vvc_reconstruct left them, the scale table's routed
    units from the scales the reference cached."""
    pic = picture(name)
    d = derive(pic)
    ret, planes, scales, twice = run_reference(lib, pic)
    assert ret == 0 and not twice, (name, ret, twice)
    table = None
    if d.tpic.model is not None:
        table = np.zeros((d.tpic.uy, d.tpic.ux), np.int16)
        for (ux, uy) in d.routed:
            table[uy, ux] = scales[(ux * pic.size_y, uy * pic.size_y)]
    return digests(pic, d, planes, table)


def oracle_digests(orc, name):
    """The same record from the oracle side."""
    pic = picture(name)
    d = derive(pic)
    planes, table, _arena = oracle_side(orc, d)
    return digests(pic, d, planes, table)


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


def first_difference(want, got):
    """None, or 'component c: n samples differ, first at (y, x): want / got'."""
    for c, (w, g) in enumerate(zip(want, got)):
        bad = np.argwhere(np.asarray(w) != np.asarray(g))
        if len(bad):
            y, x = bad[0].tolist()
            return f"component {c}: {len(bad)} samples differ, first at (y, x) = ({y}, {x}): {int(w[y, x])} / {int(g[y, x])}"
    return None


# ---------------------------------------------------------------------------------------------------------------- what the pictures reach

def census(pic, d):
    """Counts, from the unit description and the derived inputs, of what the pin is for: {premise: how often the picture has it}."""
    from collections import Counter
    n = Counter()
    ctb, sy = 1 << pic.ctb_log2, pic.size_y
    n[f"bit depth {pic.bd}"] += 1
    n[f"12 bit at range 18"] += pic.bd == 12 and pic.rbits == 18
    n[f"format {pic.idc}"] += 1
    n[f"ctu {ctb}"] += 1
    n["partial ctu right"] += pic.width % ctb != 0
    n["partial ctu below"] += pic.height % ctb != 0
    n["three slices, differing flags"] += len(pic.slices) >= 3 and len(set(pic.slices)) >= 2 and len({s[0] for s in pic.slices}) == 2 and len({s[1] for s in pic.slices}) == 2
    n["tiles"] += len(set(pic.col_bd[:-1].tolist())) > 1
    n["wavefront"] += pic.wpp
    all_cus = [(rs, cu) for rs, ctu in enumerate(pic.ctus) for cu in ctu]
    n["dual-tree all-intra picture"] += all(cu["tree_type"] != 0 for _, cu in all_cus)
    lm = pic.chroma_scale_flag
    for rs, cu in all_cus:
        sl = pic.slices[int(pic.slice_idx[rs])]
        w, h = cu["w"], cu["h"]
        luma_tbs = [b for tu in cu["tus"] for b in tu["tbs"] if b["c_idx"] == 0 and b["has"]]
        chroma_tbs = [(tu, b) for tu in cu["tus"] for b in tu["tbs"] if b["c_idx"] and b["has"]]
        if not cu["coded_flag"]:
            n["uncoded unit"] += 1
            continue
        if cu["pred_mode"] == 1:
            n["intra unit in a CTU with inter units"] += any(o["pred_mode"] == 0 for o in pic.ctus[rs])
            if cu["tree_type"] != 2:
                if w != h and not cu["mip_flag"] and 2 <= cu["mode_y"] <= 66:
                    n[f"angular {cu['mode_y']} non-square"] += 1
                n[f"reference line {cu['ref_idx']}"] += 1
                n["mip"] += cu["mip_flag"]
                if cu["isp_type"]:
                    n["isp " + ("horizontal", "vertical")[cu["isp_type"] - 1]] += 1
                    pw = cu["tus"][0]["w"]
                    if cu["isp_type"] == 2 and pw < 4:
                        unpredicted = [i for i in range(len(cu["tus"])) if i % (4 // pw)]
                        n[f"isp parts {pw} wide, residual on an unpredicted part"] += any(cu["tus"][i]["coded"][0] for i in unpredicted)
                n["bdpcm luma " + ("vertical" if cu["mode_y"] == 50 else "horizontal")] += bool(cu["bdpcm"][0] and luma_tbs)
                if cu["apply_lfnst"][0]:
                    for b in luma_tbs:
                        size = "4x4" if (b["w"], b["h"]) == (4, 4) else "8x8" if (b["w"], b["h"]) == (8, 8) else "larger"
                        n[f"lfnst {cu['lfnst_idx']} {size}"] += 1
                        n["lfnst route " + ("mip" if cu["mip_flag"] else "luma")] += 1
                for b in luma_tbs:
                    if not b["ts"] and not cu["lfnst_idx"] and pic.mts_enabled and not pic.explicit_mts_intra and not cu["mip_flag"] and not cu["isp_type"] and \
                            (4 <= b["w"] <= 16 or 4 <= b["h"] <= 16):
                        n["implicit mts"] += 1
                n[f"explicit mts {cu['mts_idx']} intra"] += bool(cu["mts_idx"] and luma_tbs)
            if cu["tree_type"] != 1 and pic.idc:
                n[f"cclm {cu['mode_c']}"] += 81 <= cu["mode_c"] <= 83
                n["bdpcm chroma " + ("vertical" if cu["mode_c"] == 50 else "horizontal")] += bool(cu["bdpcm"][1] and chroma_tbs)
                n["mip chroma direct"] += bool(cu["mip_chroma_direct"] and cu["mip_flag"])
                if cu["tree_type"] == 2 and cu["apply_lfnst"][1]:
                    for _tu, b in chroma_tbs:
                        if not b["ts"]:
                            n["lfnst route dual-tree chroma" + (" cclm" if 81 <= cu["mode_c"] <= 83 else "")] += 1
        else:
            n["inter unit with residual in a CTU the walk writes"] += bool(d.kind[rs] == 2 and (luma_tbs or chroma_tbs))
            if cu["sbt_flag"] and luma_tbs:
                n[f"sbt {'horizontal' if cu['sbt_horizontal'] else 'vertical'} pos {cu['sbt_pos']}"] += 1
            n[f"explicit mts {cu['mts_idx']} inter"] += bool(cu["mts_idx"] and luma_tbs)
            for tu, b in chroma_tbs:
                if sl[1] and lm:
                    if b["w"] * b["h"] <= 4:
                        n["chroma block of 4 samples or fewer, unscaled"] += 1
                        continue
                    xv, yv = cu["x0"] & ~(sy - 1), cu["y0"] & ~(sy - 1)
                    n["scaled, unit at the left column"] += xv == 0
                    n["scaled, unit at the top row"] += yv == 0
                    rx, ry = xv >> pic.ctb_log2, yv >> pic.ctb_log2
                    n["scaled behind a slice edge"] += bool(yv % ctb == 0 and ry and pic.slice_idx[rs] != pic.slice_idx[rs - pic.ncx])
                    n["scaled behind a tile edge"] += bool(xv % ctb == 0 and rx and pic.col_bd[rx] != pic.col_bd[rx - 1])
                    n["scaled with ctu 32"] += ctb == 32
                    if (b["x0"] // sy, b["y0"] // sy) != (cu["x0"] // sy, cu["y0"] // sy):
                        n["scaled block outside its unit's first 64x64 unit"] += 1
                        n["128-wide unit, chroma block in the second 64x64 unit"] += w == 128 and b["x0"] // sy > cu["x0"] // sy
        for b in luma_tbs:
            n["transform skip luma"] += bool(b["ts"] and not cu["bdpcm"][0])
            n["64-point block, zero-out"] += bool(not b["ts"] and max(b["w"], b["h"]) == 64)
        for tu, b in chroma_tbs:
            n["transform skip chroma"] += bool(b["ts"] and not cu["bdpcm"][1])
            if tu["joint"]:
                n[f"joint cb-cr coded {tu['coded'][1]}{tu['coded'][2]} sign {pic.joint_sign}"] += 1
    n["ctu wholly inter"] += int(np.sum(d.kind != 2))
    n["light ctu"] += int(np.sum(d.kind == 1))
    n["light ctu waits left"] += int(np.sum((d.ctus["flags"] & abi.RECON_CTU_LUMA_LEFT) != 0))
    n["light ctu waits up"] += int(np.sum((d.ctus["flags"] & abi.RECON_CTU_LUMA_UP) != 0))
    n["scaled through the table (inter neighbours)"] += d.stats["batched_scaled"]
    n["scaled in the walk (intra-written neighbour)"] += d.stats["walk_scaled"]
    return n


PREMISES = (["bit depth 8", "bit depth 10", "bit depth 12", "12 bit at range 18", "format 0", "format 1", "format 2", "format 3", "ctu 32", "ctu 64", "ctu 128",
             "partial ctu right", "partial ctu below", "three slices, differing flags", "tiles", "wavefront", "dual-tree all-intra picture"] +
            [f"angular {m} non-square" for m in range(2, 67)] +
            ["reference line 1", "reference line 2", "mip", "mip chroma direct", "isp horizontal", "isp vertical",
             "isp parts 1 wide, residual on an unpredicted part", "isp parts 2 wide, residual on an unpredicted part",
             "bdpcm luma horizontal", "bdpcm luma vertical", "bdpcm chroma horizontal", "bdpcm chroma vertical", "cclm 81", "cclm 82", "cclm 83", "uncoded unit"] +
            [f"lfnst {i} {s}" for i in (1, 2) for s in ("4x4", "8x8", "larger")] +
            ["lfnst route luma", "lfnst route mip", "lfnst route dual-tree chroma", "lfnst route dual-tree chroma cclm", "implicit mts"] +
            [f"explicit mts {i} {k}" for i in range(1, 5) for k in ("intra", "inter")] +
            [f"sbt {o} pos {p}" for o in ("horizontal", "vertical") for p in (0, 1)] +
            ["64-point block, zero-out", "transform skip luma", "transform skip chroma"] +
            [f"joint cb-cr coded {f} sign {s}" for f in ("10", "01", "11") for s in (0, 1)] +
            ["inter unit with residual in a CTU the walk writes", "intra unit in a CTU with inter units", "ctu wholly inter", "light ctu", "light ctu waits left",
             "light ctu waits up", "scaled, unit at the left column", "scaled, unit at the top row", "scaled behind a slice edge", "scaled behind a tile edge",
             "scaled through the table (inter neighbours)", "scaled in the walk (intra-written neighbour)", "scaled with ctu 32",
             "128-wide unit, chroma block in the second 64x64 unit", "chroma block of 4 samples or fewer, unscaled"])

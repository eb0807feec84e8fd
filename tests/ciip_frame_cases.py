"""Synthetic pictures with combined inter / intra (CIIP) coding units as the decoder holds them after parsing, for the CIIP stage driver
(vvc355_ciip_frame_build / _pass), in the style of affine_gpm_cases.py: the MvField table (CIIP units with pred_flag 1, 2 or 3 on a
background of 8x8 blocks that are intra — pred_flag 0 — or inter at random), one vvc355_ciip_cu per unit, two reference pictures per list,
two slices (slice 0: default weights, LMCS; slice 1: explicit weights), optionally 2 x 2 tiles, and a RECON command array with the
units' VVC355_RECON_CIIP commands among commands of other kinds.

The numpy restatement of the builder: unit_ok (which records the builder must reject), expect_jobs (the inter part of
ff_vvc_predict_ciip, libavcodec/vvc/vvc_inter.c:545-640 with :129-177, as vvc355_bipred_job tiles, with whatever addresses the caller's
maps give: host memory for the oracle, device memory to compare with), intra_weight (ciip_derive_intra_weight, :523-543, literally, on
the ctb_left / ctb_up flags of ff_vvc_decode_neighbour, vvc_ctu.c:2468-2495) and expect_cmds (the command patch)."""
import ctypes

import numpy as np

import bipred_cases as bc
import inter_frame_cases as ifc
import recon_cases
from ffvvc_amd import abi, batch

CIIP_CU_DT = np.dtype(abi.CiipCu, align=True)
BIPRED_JOB_DT = np.dtype(abi.BipredJob, align=True)
CMD = recon_cases.CMD
NO_CMD = abi.CIIP_NO_CMD
assert CIIP_CU_DT.itemsize == 32 and BIPRED_JOB_DT.itemsize == 104 and CMD.itemsize == 40

# the CIIP units of a 64x64 area (x, y, w, h); what they leave uncovered is background.  Areas of CTUs of 64 and 128 samples.
L64 = [
    [(0, 0, 64, 64)],
    [(0, 0, 64, 16), (0, 16, 32, 8), (32, 16, 32, 8), (0, 24, 16, 4), (16, 24, 4, 16), (24, 24, 8, 8), (32, 32, 32, 32), (0, 48, 16, 16)],
    [(0, 0, 16, 16), (32, 0, 8, 8), (48, 0, 16, 4), (0, 32, 4, 16), (8, 32, 8, 8), (32, 32, 32, 8), (48, 48, 16, 16), (16, 56, 16, 4), (0, 60, 16, 4)],
    [(0, 0, 32, 32), (32, 0, 32, 8), (32, 8, 8, 8), (40, 8, 4, 16), (32, 32, 16, 16), (48, 32, 16, 4), (0, 32, 32, 32), (60, 40, 4, 16), (48, 56, 8, 8)],
]
# the same for CTUs of 32 samples, per 32x32 area
L32 = [
    [(0, 0, 32, 32)],
    [(0, 0, 32, 8), (0, 8, 4, 16), (4, 8, 16, 4), (8, 16, 8, 8), (16, 16, 16, 16)],
    [(0, 0, 8, 8), (16, 0, 16, 4), (0, 16, 4, 16), (16, 16, 16, 16)],
    [(0, 0, 16, 16), (16, 0, 16, 16), (0, 16, 32, 8), (0, 24, 32, 8)],
]

# the GPU test's picture list: (bd, chroma_format_idc, ctb_log2, width, height, tiles, motion range in 1/16 sample)
CASES = [(10, 1, 6, 256, 192, True, 20 * 16), (8, 3, 5, 128, 96, False, 20 * 16), (12, 2, 7, 256, 192, False, 20 * 16),
         (10, 0, 6, 128, 128, False, 20 * 16), (10, 1, 6, 128, 128, False, 300 * 16)]
FMT = {0: (0, 0), 1: (1, 1), 2: (1, 0), 3: (0, 0)}          # chroma_format_idc -> (hs, vs)
SEEDS = [0xC1230, 0xC1201, 0xC11F2, 0xC11F3, 0xC1224]


def tiles_of(cb_w, cb_h, hs, vs, chroma):
    """The <= 16x16 tiles of a unit per present component: (c, tx, ty, tw, th) in the component's samples, in job order."""
    out = []
    for c in range(3 if chroma else 1):
        sx, sy = (hs, vs) if c else (0, 0)
        w, h = cb_w >> sx, cb_h >> sy
        tw, th = min(w, 16), min(h, 16)
        out += [(c, tx, ty, tw, th) for ty in range(0, h, th) for tx in range(0, w, tw)]
    return out


def n_tiles(cb_w, cb_h, hs, vs, chroma):
    n = ((cb_w + 15) // 16) * ((cb_h + 15) // 16)
    if chroma:
        n += 2 * (((cb_w >> hs) + 15) // 16) * (((cb_h >> vs) + 15) // 16)
    return n


def region_len(cb_w, cb_h, hs, vs, chroma):
    """Pixels of a unit's scratch region: luma, and Cb + Cr where the chroma is blended (wc > 2, do_ciip vvc_inter.c:590)."""
    wc, hc = cb_w >> hs, cb_h >> vs
    return cb_w * cb_h + (2 * wc * hc if chroma and wc > 2 else 0)


def part_offset(cb_w, cb_h, hs, vs, c):
    """Pixel offset of component c inside the unit's region."""
    return 0 if c == 0 else cb_w * cb_h + (c - 1) * (cb_w >> hs) * (cb_h >> vs)


def make_slices(rng):
    """slice 0: default weighting, LMCS on; slice 1: explicit weighted bi- and uni-prediction, no LMCS (as inter_frame_cases.py)."""
    slices = (abi.InterSlice * 2)()
    slices[0].lmcs_used = 1
    s1 = slices[1]
    s1.weighted_pred, s1.weighted_bipred = 0, 1
    s1.log2_denom[0], s1.log2_denom[1] = 6, 5
    for l in range(2):
        for c in range(3):
            for r in range(16):
                s1.weight[l][c][r] = int(rng.integers(-32, 96))
                s1.offset[l][c][r] = int(rng.integers(-20, 21))
    return slices


def random_motion(rng, mv_range, hpel):
    """An MvField of a CIIP unit: (pred_flag, ref_idx[2], bcw_idx, mv[2][2])."""
    pred_flag = int(rng.choice([1, 2, 3, 3]))
    ref_idx = rng.integers(0, 2, size=2)
    bcw = int(rng.integers(1, 5)) if pred_flag == 3 and rng.random() < 0.4 else 0
    mv = rng.integers(-mv_range, mv_range + 1, size=(2, 2))
    if hpel:
        mv = mv // 8 * 8
    return pred_flag, [ref_idx[0] if pred_flag & 1 else -1, ref_idx[1] if pred_flag & 2 else -1], bcw, mv


def fill_background(rng, mvf):
    """8x8 blocks that are intra (pred_flag 0) or inter at random."""
    th, tw = mvf.shape
    for y in range(0, th, 2):
        for x in range(0, tw, 2):
            pf = int(rng.choice([0, 0, 1, 2, 3]))
            blk = mvf[y:y + 2, x:x + 2]
            blk["pred_flag"] = pf
            blk["ref_idx"] = [int(rng.integers(0, 2)) if pf & 1 else -1, int(rng.integers(0, 2)) if pf & 2 else -1]
            blk["mv"] = rng.integers(-64, 65, size=(2, 2))


class CiipPicture:
    """What the builder reads: geometry, MvField table, slices, the CTU tables, the records and the command array (cmds, as uploaded:
    resid and joint of the CIIP commands hold garbage the builder must replace)."""

    def __init__(self, width, height, ctb_log2, idc, isz):
        self.width, self.height, self.ctb_log2, self.idc, self.isz = width, height, ctb_log2, idc, isz
        self.hs, self.vs = FMT[idc]
        self.chroma = idc != 0
        ctb = 1 << ctb_log2
        self.ncx, self.ncy = (width + ctb - 1) // ctb, (height + ctb - 1) // ctb
        self.mvf = np.zeros((height // 4, width // 4), ifc.MVF_DT)
        self.slice_idx = np.zeros(self.ncx * self.ncy, np.int16)
        self.col_bd = np.array([0] * self.ncx + [self.ncx], np.int16)
        self.row_bd = np.array([0] * self.ncy + [self.ncy], np.int16)
        self.slices = None
        self.n_slices = 2
        self.cus = np.zeros(0, CIIP_CU_DT)
        self.n_jobs = 0
        self.scratch_len = 0
        self.cmds = np.zeros(0, CMD)

    def set_records(self, rng, units, gaps=True):
        """units: (x0, y0, w, h, hpel, slice) -> records with running first_job / scratch_off sums (random gaps between the regions)."""
        self.cus = np.zeros(len(units), CIIP_CU_DT)
        first = off = 0
        for i, (x, y, w, h, hpel, sl) in enumerate(units):
            r = self.cus[i]
            off += int(rng.integers(0, 8)) if gaps else 0
            r["x0"], r["y0"], r["cb_width"], r["cb_height"], r["hpel_if_idx"], r["slice"], r["first_job"], r["scratch_off"] = x, y, w, h, hpel, sl, first, off
            r["cmd"] = NO_CMD
            first += n_tiles(w, h, self.hs, self.vs, self.chroma)
            off += region_len(w, h, self.hs, self.vs, self.chroma)
        self.n_jobs, self.scratch_len = first, off + 5

    def frame(self, pic, cus_ptr, jobs_ptr, scratch_ptr, cmds_ptr=0, slice_ptr=0, col_ptr=0, row_ptr=0):
        return abi.CiipFrame(pic=pic, cus=cus_ptr, jobs=jobs_ptr, scratch=scratch_ptr, cmds=cmds_ptr, slice_idx=slice_ptr, ctb_to_col_bd=col_ptr,
                             ctb_to_row_bd=row_ptr, n_cus=len(self.cus), n_jobs=self.n_jobs, scratch_len=self.scratch_len, n_slices=self.n_slices,
                             n_cmds=len(self.cmds), ctb_width=self.ncx, ctb_height=self.ncy, ctb_log2=self.ctb_log2)

    def pic(self, dst_ptrs, dst_strides, mvf_ptr, refs_ptr, slices_ptr, lut_ptr):
        f = abi.InterFrame()
        for c in range(3):
            f.dst[c], f.dst_stride[c] = dst_ptrs[c], dst_strides[c]
        f.mvf, f.refs, f.slices, f.lmcs_fwd_lut = mvf_ptr, refs_ptr, slices_ptr, lut_ptr
        f.mvf_stride, f.width, f.height = self.width // 4, self.width, self.height
        f.hs, f.vs, f.chroma_format_idc, f.pixel_shift = self.hs, self.vs, self.idc, int(self.isz == 2)
        return f


def case_picture(i, seed=None):
    """Picture i of CASES, deterministic (SEEDS: chosen so that every picture holds what test_ciip_frame_cpu.py asks of it)."""
    bd, idc, ctb_log2, width, height, tiles, mv_range = CASES[i]
    rng = np.random.default_rng(SEEDS[i] if seed is None else seed)
    p = CiipPicture(width, height, ctb_log2, idc, 1 if bd == 8 else 2)
    p.bd, p.mv_range = bd, mv_range
    ctb = 1 << ctb_log2
    # two slices: the first CTU row, and the rest; tiles: 2 x 2, the row edge NOT on the slice edge
    p.slice_idx[:] = (np.arange(p.ncx * p.ncy) // p.ncx > 0).astype(np.int16)
    if tiles:
        assert p.ncx >= 4 and p.ncy >= 3
        p.col_bd = np.array([0 if x < 2 else 2 for x in range(p.ncx)] + [p.ncx], np.int16)
        p.row_bd = np.array([0 if y < 2 else 2 for y in range(p.ncy)] + [p.ncy], np.int16)
    p.slices = make_slices(rng)
    fill_background(rng, p.mvf)
    area, layouts = (64, L64) if ctb >= 64 else (32, L32)
    units = []
    per_row = width // area
    for a in range(per_row * (height // area)):
        ax, ay = (a % per_row) * area, (a // per_row) * area
        for (dx, dy, w, h) in layouts[(a + a // per_row + i) % len(layouts)]:
            x, y = ax + dx, ay + dy
            hpel = int(rng.random() < 0.2)
            pf, ref_idx, bcw, mv = random_motion(rng, mv_range, hpel)
            blk = p.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
            blk["mv"], blk["ref_idx"], blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"], blk["ciip_flag"] = mv, ref_idx, hpel, bcw, pf, 1
            units.append((x, y, w, h, hpel, int(p.slice_idx[(y >> ctb_log2) * p.ncx + (x >> ctb_log2)])))
    p.set_records(rng, units)
    build_commands(rng, p)
    return p


def _cmd(kind, c, x, y, w, h, resid=0, joint=0):
    return recon_cases.ReconWork._cmd(kind, c, x, y, w, h, x, y, w, h, resid=resid, joint=joint)


def build_commands(rng, p):
    """The units' command lists as the RECON pass takes them (PRED + CIIP per blended component, then the MARKs), with a RESID command of
    an unrelated block now and then.  resid / joint of the CIIP commands hold garbage.  Deliberate oddities, by unit index: every 7th unit
    does not name its Cr command; every 5th unit's Cb command has another width than the record; every 11th names its luma PRED command
    instead of the CIIP one; every 13th names an index past the array."""
    cmds = []
    for u, cu in enumerate(p.cus):
        x, y, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
        if rng.random() < 0.3:
            cmds.append(_cmd(abi.RECON_RESID, 0, x, y, 4, 4, resid=int(rng.integers(1, 1 << 40)), joint=int(rng.integers(0, 8))))
        for c in range(3 if p.chroma else 1):
            if c and (w >> p.hs) <= 2:
                continue
            cmds.append(_cmd(abi.RECON_PRED, c, x, y, w, h))
            named = len(cmds)
            cw = w // 2 if (c == 1 and u % 5 == 4) else w
            cmds.append(_cmd(abi.RECON_CIIP, c, x, y, cw, h, resid=int(rng.integers(1, 1 << 40)), joint=int(rng.integers(4, 256))))
            if c == 2 and u % 7 == 6:
                continue
            if c == 0 and u % 11 == 10:
                named -= 1
            if c == 0 and u % 13 == 12:
                named = 1 << 30
            p.cus[u]["cmd"][c] = named
        cmds.append(_cmd(abi.RECON_MARK, 0, x, y, w, h))
        cmds.append(_cmd(abi.RECON_MARK, 1, x, y, w, h))
    p.cmds = np.array(cmds, CMD)
    # the pad bytes belong to the RECON pass; whatever is there must survive the builder
    p.cmds.view(np.uint8).reshape(len(cmds), -1)[:, 34:40] = rng.integers(0, 256, size=(len(cmds), 6), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the restatement

def unit_ok(p, cu, n_jobs=None, scratch_len=None):
    """The records the builder accepts (include/vvc_mi355.h, vvc355_ciip_cu)."""
    n_jobs = p.n_jobs if n_jobs is None else n_jobs
    scratch_len = p.scratch_len if scratch_len is None else scratch_len
    x0, y0, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
    if x0 % 4 or y0 % 4 or w not in (4, 8, 16, 32, 64) or h not in (4, 8, 16, 32, 64) or w * h < 64:
        return False
    L = p.ctb_log2
    if x0 < 0 or y0 < 0 or x0 + w > p.width or y0 + h > p.height or x0 >> L != (x0 + w - 1) >> L or y0 >> L != (y0 + h - 1) >> L:
        return False
    if int(cu["slice"]) >= p.n_slices or int(cu["first_job"]) + n_tiles(w, h, p.hs, p.vs, p.chroma) > n_jobs:
        return False
    if int(cu["scratch_off"]) + region_len(w, h, p.hs, p.vs, p.chroma) > scratch_len:
        return False
    m = p.mvf[y0 >> 2, x0 >> 2]
    pf = int(m["pred_flag"])
    return 1 <= pf <= 3 and all(not (pf & (1 << l)) or 0 <= int(m["ref_idx"][l]) <= 15 for l in range(2))


def weights(slices, sl, m, c):
    """derive_weight (dmvr_flag 0) with cu->ciip_flag set / derive_weight_uni, vvc_inter.c:129-177: (weight_flag, denom, w0, w1, o0, o1)."""
    s = slices[sl]
    pf, ref_idx, bcw = int(m["pred_flag"]), m["ref_idx"], int(m["bcw_idx"])
    weight_flag = bool(s.weighted_pred or s.weighted_bipred)
    if pf == 3:
        if (not weight_flag and not bcw) or bcw:                          # :158, (bcw_idx && lc->cu->ciip_flag)
            return 0, 0, 0, 0, 0, 0
        r0, r1 = int(ref_idx[0]), int(ref_idx[1])
        return 1, s.log2_denom[c > 0], s.weight[0][c][r0], s.weight[1][c][r1], s.offset[0][c][r0], s.offset[1][c][r1]
    if not weight_flag:
        return 0, 0, 0, 0, 0, 0
    lx = pf - 1
    r = int(ref_idx[lx])
    return 1, s.log2_denom[c > 0], s.weight[lx][c][r], 0, s.offset[lx][c][r], 0


def expect_jobs(p, plane, ref, scratch, lut, n_jobs=None, scratch_len=None):
    """The job array: plane(c) -> (address, stride) of the current picture, ref(l, r, c) -> (address, stride), scratch = address of the
    scratch buffer, lut = address of the forward map.  Slots of rejected records, and slots no record claims, stay zero."""
    n_jobs = p.n_jobs if n_jobs is None else n_jobs
    jobs = np.zeros(n_jobs, BIPRED_JOB_DT)
    for cu in p.cus:
        if not unit_ok(p, cu, n_jobs, scratch_len):
            continue
        x0, y0, cbw, cbh, sl = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height", "slice"))
        mv = p.mvf[y0 >> 2, x0 >> 2]                                                             # ff_vvc_get_mvf at the unit's origin
        wc = cbw >> p.hs
        for i, (c, tx, ty, tw, th) in enumerate(tiles_of(cbw, cbh, p.hs, p.vs, p.chroma)):
            hs, vs = (p.hs, p.vs) if c else (0, 0)
            j = jobs[int(cu["first_job"]) + i]
            x, y = (x0 >> hs) + tx, (y0 >> vs) + ty
            if c and wc <= 2:                                                                    # no blend (:590): straight to the picture
                base, stride = plane(c)
                j["dst"], j["dst_stride"] = base + y * stride + x * p.isz, stride
            else:
                w = cbw >> hs
                j["dst"] = scratch + (int(cu["scratch_off"]) + part_offset(cbw, cbh, p.hs, p.vs, c) + ty * w + tx) * p.isz
                j["dst_stride"] = w * p.isz
            for l in range(2):
                if int(mv["pred_flag"]) & (1 << l):
                    j[f"ref{l}"], j[f"ref{l}_stride"] = ref(l, int(mv["ref_idx"][l]), c)
                    j["mv"][2 * l:2 * l + 2] = mv["mv"][l]
            j["x"], j["y"], j["w"], j["h"] = x, y, tw, th
            j["pic_w"], j["pic_h"] = p.width >> hs, p.height >> vs
            j["chroma"], j["hs"], j["vs"] = int(c > 0), p.hs, p.vs
            j["hf_idx"] = j["vf_idx"] = 0 if c else int(cu["hpel_if_idx"])                      # pred_regular_luma :548-549, chroma: set 0
            j["pred_flag"] = mv["pred_flag"]
            j["weight_flag"], j["denom"], j["w0"], j["w1"], j["o0"], j["o1"] = weights(p.slices, sl, mv, c)
            j["lmcs_lut"] = lut if (c == 0 and p.slices[sl].lmcs_used) else 0                   # :573-574
    return jobs


def neighbour_flags(p, rx, ry):
    """(ctb_left_flag, ctb_up_flag) of ff_vvc_decode_neighbour (vvc_ctu.c:2468-2495)."""
    rs = ry * p.ncx + rx
    left_tile = rx > 0 and p.col_bd[rx] != p.col_bd[rx - 1]
    upper_tile = ry > 0 and p.row_bd[ry] != p.row_bd[ry - 1]
    upper_slice = ry > 0 and p.slice_idx[rs] != p.slice_idx[rs - p.ncx]
    return bool(rx > 0 and not left_tile), bool(ry > 0 and not upper_tile and not upper_slice)


def intra_weight(p, x0, y0, width, height):
    """ciip_derive_intra_weight (vvc_inter.c:523-543)."""
    ctb_left, ctb_up = neighbour_flags(p, x0 >> p.ctb_log2, y0 >> p.ctb_log2)
    x0b, y0b = x0 & ((1 << p.ctb_log2) - 1), y0 & ((1 << p.ctb_log2) - 1)
    available_l = ctb_left or x0b
    available_u = ctb_up or y0b
    w = 1
    if available_u and p.mvf[(y0 - 1) >> 2, (x0 - 1 + width) >> 2]["pred_flag"] == 0:
        w += 1
    if available_l and p.mvf[(y0 - 1 + height) >> 2, (x0 - 1) >> 2]["pred_flag"] == 0:
        w += 1
    return w


def unit_weights(p):
    return np.array([intra_weight(p, int(cu["x0"]), int(cu["y0"]), int(cu["cb_width"]), int(cu["cb_height"])) for cu in p.cus], np.int64)


def expect_cmds(p, scratch, n_jobs=None, scratch_len=None):
    """The command array after the builder: resid / joint of the commands the accepted records name and that pass the identity check."""
    out = p.cmds.copy()
    for cu in p.cus:
        if not unit_ok(p, cu, n_jobs, scratch_len):
            continue
        x0, y0, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
        for c in range(3 if p.chroma else 1):
            if c and (w >> p.hs) <= 2:
                continue
            idx = int(cu["cmd"][c])
            if idx >= len(out):
                continue
            k = out[idx]
            if k["kind"] != abi.RECON_CIIP or k["c_idx"] != c or (int(k["x0"]), int(k["y0"]), int(k["w"]), int(k["h"])) != (x0, y0, w, h):
                continue
            k["resid"] = scratch + (int(cu["scratch_off"]) + part_offset(w, h, p.hs, p.vs, c)) * p.isz
            k["joint"] = intra_weight(p, x0, y0, w, h)
    return out


def region_mask(p, n_jobs=None, scratch_len=None):
    """Which scratch pixels belong to an accepted unit's region."""
    m = np.zeros(p.scratch_len if scratch_len is None else scratch_len, bool)
    for cu in p.cus:
        if unit_ok(p, cu, n_jobs, scratch_len):
            off = int(cu["scratch_off"])
            m[off:off + region_len(int(cu["cb_width"]), int(cu["cb_height"]), p.hs, p.vs, p.chroma)] = True
    return m


def plane_mask(p, c, n_jobs=None, scratch_len=None):
    """Which samples of chroma plane c the pass writes: the wc <= 2 chroma blocks of accepted units."""
    m = np.zeros((p.height >> p.vs, p.width >> p.hs), bool)
    for cu in p.cus:
        w, h = int(cu["cb_width"]), int(cu["cb_height"])
        if p.chroma and c and unit_ok(p, cu, n_jobs, scratch_len) and (w >> p.hs) <= 2:
            x, y = int(cu["x0"]) >> p.hs, int(cu["y0"]) >> p.vs
            m[y:y + (h >> p.vs), x:x + (w >> p.hs)] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- shared inputs / plumbing

def ref_table(ptrs, strides):
    t = (abi.RefPic * 32)()
    for l in range(2):
        for r in range(2):
            for c in range(3):
                t[l * 16 + r].plane[c] = ptrs[l][r][c]
                t[l * 16 + r].stride[c] = strides[c]
    return t


def pictures(rng, p, bd):
    """Reference pictures [list][ref][component] and the forward LMCS map."""
    dims = [(p.width, p.height)] + [(p.width >> p.hs, p.height >> p.vs)] * 2
    base = [bc.smooth_picture(rng, ph, pw, bd) for (pw, ph) in dims]
    refs = [[[bc.shifted(base[c], (2 * l - 1) * (r + 1) >> (p.hs if c else 0), (1 - 2 * l) * (r + 2) >> (p.vs if c else 0)) for c in range(3)]
             for r in range(2)] for l in range(2)]
    lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)      # fc->ps.lmcs.fwd_lut
    return dims, refs, lut


def call(fn, bd, arr):
    """Run an oracle block function on every job of a structured array."""
    saved = fn.argtypes, fn.restype
    fn.argtypes, fn.restype = [ctypes.c_int, ctypes.c_void_p], None
    try:
        for i in range(len(arr)):
            fn(bd, arr[i:i + 1].ctypes.data)
    finally:
        fn.argtypes, fn.restype = saved


def oracle_run(orc, p, bd, dims, refs, lut, sentinel, n_jobs=None, scratch_len=None):
    """orc_bipred_block on the expected jobs over host memory: (jobs, scratch, planes)."""
    dt = refs[0][0][0].dtype
    scratch = np.full(p.scratch_len if scratch_len is None else scratch_len, sentinel, dt)
    planes = [np.full((ph, pw), sentinel, dt) for (pw, ph) in dims]
    jobs = expect_jobs(p, lambda c: (planes[c].ctypes.data, dims[c][0] * p.isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * p.isz),
                       scratch.ctypes.data, lut.ctypes.data, n_jobs, scratch_len)
    call(orc.orc_bipred_block, bd, jobs[jobs["w"] > 0])
    return jobs, scratch, planes


class DeviceRun:
    """The picture on the device and one vvc355_ciip_frame_pass (or _build) over it."""

    def __init__(self, dev, p, bd, dims, refs, lut, sentinel, with_cmds=True, n_jobs=None, scratch_len=None):
        self.dev, self.p, self.bd, self.dims = dev, p, bd, dims
        dt = refs[0][0][0].dtype
        self.dt = dt
        self.n_jobs = p.n_jobs if n_jobs is None else n_jobs
        self.scratch_len = p.scratch_len if scratch_len is None else scratch_len
        self.pitches = [batch.plane_pitch(d[0], p.isz) for d in dims]
        self.d_dst = [batch.DeviceBuffer.from_host(batch.to_pitched(np.full((ph, pw), sentinel, dt))) for (pw, ph) in dims]
        self.d_ref = [[[batch.DeviceBuffer.from_host(batch.to_pitched(refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
        t_refs = ref_table([[[self.d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], self.pitches)
        self.d_reft = batch.DeviceBuffer.from_host(np.frombuffer(bytes(t_refs), np.uint8))
        self.d_mvf = batch.DeviceBuffer.from_host(p.mvf.view(np.uint8))
        self.d_sl = batch.DeviceBuffer.from_host(np.frombuffer(bytes(p.slices), np.uint8))
        self.d_lut = batch.DeviceBuffer.from_host(lut)
        self.d_cus = batch.DeviceBuffer.from_host(p.cus.view(np.uint8))
        self.d_jobs = batch.DeviceBuffer.from_host(np.full(max(1, self.n_jobs) * BIPRED_JOB_DT.itemsize, 0xA5, np.uint8))
        self.d_scratch = batch.DeviceBuffer.from_host(np.full(self.scratch_len, sentinel, dt))
        self.with_cmds = with_cmds
        if with_cmds:
            self.d_cmds = batch.DeviceBuffer.from_host(p.cmds.view(np.uint8))
            self.d_tabs = [batch.DeviceBuffer.from_host(a) for a in (p.slice_idx, p.col_bd, p.row_bd)]
        pic = p.pic([b.ptr for b in self.d_dst], self.pitches, self.d_mvf.ptr, self.d_reft.ptr, self.d_sl.ptr, self.d_lut.ptr)
        self.frame = p.frame(pic, self.d_cus.ptr, self.d_jobs.ptr, self.d_scratch.ptr, *((self.d_cmds.ptr, *(t.ptr for t in self.d_tabs)) if with_cmds else ()))
        self.frame.n_jobs, self.frame.scratch_len = self.n_jobs, self.scratch_len
        if not with_cmds:
            self.frame.n_cmds = 0
        self.d_frame = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.frame), np.uint8))

    def run(self, stream=None):
        return self.dev.vvc355_ciip_frame_pass(stream, self.bd, self.d_frame.ptr, ctypes.addressof(self.frame))

    def expected_jobs(self):
        return expect_jobs(self.p, lambda c: (self.d_dst[c].ptr, self.pitches[c]), lambda l, r, c: (self.d_ref[l][r][c].ptr, self.pitches[c]),
                           self.d_scratch.ptr, self.d_lut.ptr, self.n_jobs, self.scratch_len)

    def jobs(self):
        return self.d_jobs.to_host(BIPRED_JOB_DT, (self.n_jobs,))

    def scratch(self):
        return self.d_scratch.to_host(self.dt, (self.scratch_len,))

    def plane(self, c):
        return self.d_dst[c].to_host(self.dt, (self.dims[c][1], self.pitches[c] // self.p.isz))[:, :self.dims[c][0]]

    def cmds(self):
        return self.d_cmds.to_host(CMD, (len(self.p.cmds),))


# ---------------------------------------------------------------------------------------------------------------- malformed records

MALFORMED = ("misaligned origin", "side of 12", "area 32", "crossing a CTU edge", "outside the picture", "slice out of range",
             "region past scratch_len", "first_job past n_jobs", "pred_flag 0", "ref_idx 16")


def with_malformed(p):
    """(picture with the ten malformed records of MALFORMED mixed into p's list, n_jobs, index of each malformed record).  The MvField table
    is shared with p (one background entry gets ref_idx 16 — call this before anything is derived from p).  Every malformed record names
    CIIP commands of its own, appended to the array, whose geometry IS the record's: only the rejection keeps them unpatched."""
    import copy
    q = copy.copy(p)
    ctb = 1 << p.ctb_log2
    cf = p.mvf["ciip_flag"]
    free = (cf[::2, ::2] | cf[1::2, ::2] | cf[::2, 1::2] | cf[1::2, 1::2]) == 0                               # 8x8 blocks no CIIP unit touches
    intra = np.argwhere((p.mvf["pred_flag"][::2, ::2] == 0) & free) * 8                                        # background, intra
    inter = np.argwhere((p.mvf["pred_flag"][::2, ::2] == 1) & free) * 8                                        # ... uni-predicted from list 0
    iy, ix = (int(v) for v in intra[len(intra) // 2])
    py, px = (int(v) for v in inter[len(inter) // 2])
    p.mvf[py // 4:py // 4 + 2, px // 4:px // 4 + 2]["ref_idx"][..., 0] = 16
    good = p.cus[0]
    gx, gy = int(good["x0"]), int(good["y0"])
    bad = {
        "misaligned origin": (gx + 2, gy, 8, 8, 0),
        "side of 12": (gx, gy, 12, 8, 0),
        "area 32": (gx, gy, 4, 8, 0),
        "crossing a CTU edge": (ctb - 8, 0, 16, 8, 0),
        "outside the picture": (p.width, 0, 8, 8, 0),
        "slice out of range": (gx, gy, 8, 8, p.n_slices),
        "region past scratch_len": (gx, gy, 8, 8, 0),
        "pred_flag 0": (ix, iy, 8, 8, 0),
        "ref_idx 16": (px, py, 8, 8, 0),
        "first_job past n_jobs": (gx, gy, 16, 16, 0),
    }
    order = [k for k in MALFORMED if k != "first_job past n_jobs"]
    recs, where = [], {}
    step = max(1, len(p.cus) // len(order))
    for i, cu in enumerate(p.cus):
        if i % step == 0 and i // step < len(order):
            where[order[i // step]] = len(recs)
            recs.append(None)
        recs.append(cu)
    where["first_job past n_jobs"] = len(recs)
    recs.append(None)
    names = {v: k for k, v in where.items()}
    q.cus = np.zeros(len(recs), CIIP_CU_DT)
    extra = []
    first = off = 0
    for i, r in enumerate(recs):
        if r is not None:
            q.cus[i] = r
        o = q.cus[i]
        if r is not None:
            w, h = int(r["cb_width"]), int(r["cb_height"])
        else:
            x, y, w, h, sl = bad[names[i]]
            o["x0"], o["y0"], o["cb_width"], o["cb_height"], o["slice"] = x, y, w, h, sl
            for c in range(3 if p.chroma else 1):
                o["cmd"][c] = len(p.cmds) + len(extra)
                extra.append(_cmd(abi.RECON_CIIP, c, x, y, w, h, resid=0x1234, joint=77))
        o["first_job"], o["scratch_off"] = first, off
        first += n_tiles(w, h, p.hs, p.vs, p.chroma)
        off += region_len(w, h, p.hs, p.vs, p.chroma) + 3
    q.scratch_len = off + 5
    q.cus[where["region past scratch_len"]]["scratch_off"] = q.scratch_len - 10
    q.n_jobs = first - 1                                      # the last record's tiles end one slot past the array
    q.cmds = np.concatenate([p.cmds, np.array(extra, CMD)])
    return q, where


# ---------------------------------------------------------------------------------------------------------------- end to end

def e2e_work():
    """A mixed picture (intra, inter and CIIP units; two slices, tiles, chroma residual scaling) as recon_cases builds it, and the CIIP
    picture that goes with it: the MvField table (intra units pred_flag 0, every other unit inter, CIIP units with their motion) and one
    record per CIIP unit that names the unit's commands in work.cmds."""
    bd, width, height, ctb_log2 = 10, 256, 192, 6
    rng = np.random.default_rng(0xC11FE2E)
    work = recon_cases.ReconWork(rng, width, height, ctb_log2, 1, 1, intra_frac=0.4, ciip_frac=0.5, n_slices=2, tiles=True, lmcs=True)
    p = CiipPicture(width, height, ctb_log2, 1, 2)
    p.bd = bd
    p.slice_idx, p.col_bd, p.row_bd = work.slice_idx, work.col_bd, work.row_bd
    p.slices = make_slices(rng)
    # every unit inter ...
    for y in range(0, height // 4, 2):
        for x in range(0, width // 4, 2):
            pf, ref_idx, bcw, mv = random_motion(rng, 64, 0)
            blk = p.mvf[y:y + 2, x:x + 2]
            blk["mv"], blk["ref_idx"], blk["bcw_idx"], blk["pred_flag"] = mv, ref_idx, bcw, pf
    # ... but the intra ones: the coding units that have an intra prediction command and are not CIIP
    ciip_rects = {(x, y, w, h) for (_c, x, y, w, h, _off, _k) in work.ciip}
    for k in work.cmds[np.isin(work.cmds["kind"], (abi.RECON_PRED, abi.RECON_CCLM))]:
        rect = (int(k["cu_x0"]), int(k["cu_y0"]), int(k["cb_width"]), int(k["cb_height"]))
        if rect not in ciip_rects:
            p.mvf[rect[1] // 4:(rect[1] + rect[3]) // 4, rect[0] // 4:(rect[0] + rect[2]) // 4] = np.zeros((), ifc.MVF_DT)
    units, named = [], []
    for (c, x, y, w, h, off, k) in work.ciip:
        if c == 0:
            hpel = int(rng.random() < 0.2)
            pf, ref_idx, bcw, mv = random_motion(rng, 20 * 16, hpel)
            blk = p.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
            blk["mv"], blk["ref_idx"], blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"], blk["ciip_flag"] = mv, ref_idx, hpel, bcw, pf, 1
            units.append((x, y, w, h, hpel, min(1, int(p.slice_idx[(y >> ctb_log2) * p.ncx + (x >> ctb_log2)])), off))
            named.append([NO_CMD] * 3)
        assert (x, y, w, h) == units[-1][:4]
        named[-1][c] = k
    p.set_records(rng, [u[:6] for u in units], gaps=False)
    p.cus["scratch_off"] = [u[6] for u in units]                # recon_cases lays a unit's components out back to back: the record's layout
    p.cus["cmd"] = named
    p.scratch_len = work.ciip_len
    p.cmds = work.cmds
    return work, p

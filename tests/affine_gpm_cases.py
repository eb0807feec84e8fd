"""A synthetic picture with affine and geometric-partition (GPM) coding units as the decoder holds it after parsing, for the affine and
GPM stage drivers (vvc355_affine_frame_pass / vvc355_gpm_frame_pass), in the style of inter_frame_cases.py: the MvField table (one
entry per 4x4 luma block; affine units with motion that varies per 4x4 sub-block), one record per coding unit (vvc355_affine_cu with
the PROF switches and offsets, vvc355_gpm_cu with the partition and the two parts' motion), two reference pictures per list and two
slices (default weights with LMCS; explicit weights without).

expect_affine / expect_gpm restate the reference's walks, pred_affine_blk and pred_gpm_blk (libavcodec/vvc/vvc_inter.c), and
produce the job arrays with whatever addresses the caller's maps give: host planes for the oracle, device planes to compare with."""
import ctypes

import numpy as np

import inter_frame_cases as ifc
from ffvvc_amd import abi

AFFINE, GPM = "A", "G"
# layouts of a 64x64 area: (kind, x, y, w, h); areas not covered keep the picture's sentinel
LAYOUTS = [
    [(AFFINE, 0, 0, 32, 32), (GPM, 32, 0, 32, 32), (AFFINE, 32, 32, 32, 32)] + [(GPM, x, 32 + y, 8, 8) for y in range(0, 32, 8) for x in range(0, 32, 8)],
    [(AFFINE, 0, 0, 16, 64), (GPM, 16, 0, 16, 64), (AFFINE, 32, 0, 32, 16), (GPM, 32, 16, 32, 8), (GPM, 32, 24, 32, 8), (GPM, 32, 32, 8, 32),
     (GPM, 40, 32, 8, 32), (AFFINE, 48, 32, 16, 16), (GPM, 48, 48, 8, 8), (GPM, 56, 48, 8, 8), (GPM, 48, 56, 8, 8)],
    [((AFFINE, GPM, None)[(x // 16 + y // 16) % 3], x, y, 16, 16) for y in range(0, 64, 16) for x in range(0, 64, 16)],
    [(GPM, 0, 0, 64, 16), (AFFINE, 0, 16, 64, 32), (GPM, 0, 48, 32, 16), (GPM, 32, 48, 16, 16), (AFFINE, 48, 48, 16, 16)],
    [(GPM, 0, 0, 64, 64)],
    [(AFFINE, 0, 0, 64, 64)],
    [(AFFINE, 0, 0, 32, 16), (AFFINE, 0, 16, 32, 16), (GPM, 32, 0, 16, 32), (GPM, 48, 0, 16, 8), (GPM, 48, 8, 8, 16), (AFFINE, 0, 32, 16, 32),
     (GPM, 16, 32, 16, 32), (GPM, 32, 32, 32, 8), (AFFINE, 32, 40, 32, 16), (GPM, 32, 56, 16, 8)],
]
AFFINE_CU_DT = np.dtype(abi.AffineCu, align=True)
GPM_CU_DT = np.dtype(abi.GpmCu, align=True)
AFFINE_JOB_DT = np.dtype(abi.AffineJob, align=True)
BIPRED_JOB_DT = np.dtype(abi.BipredJob, align=True)
GPM_JOB_DT = np.dtype(abi.GpmJob, align=True)
assert AFFINE_CU_DT.itemsize == 144 and GPM_CU_DT.itemsize == 64


def gpm_tiles(cb_w, cb_h, hs, vs, chroma):
    """The <= 16x16 tiles of a GPM unit per component: (c, x, y, w, h) in component samples relative to the unit, jobs in this order."""
    out = []
    for c in range(3 if chroma else 1):
        sx, sy = (hs, vs) if c else (0, 0)
        w, h = cb_w >> sx, cb_h >> sy
        tw, th = min(w, 16), min(h, 16)
        out += [(c, tx, ty, tw, th) for ty in range(0, h, th) for tx in range(0, w, tw)]
    return out


def round_half(v):
    """ff_vvc_round_mv(mv, 0, 1) (vvc_mvs.c:1739)."""
    return (v + 1 - (v >= 0)) >> 1


class AffineGpmWork:
    def __init__(self, rng, width, height, hs, vs, chroma, isz, mv_range=20 * 16):
        assert width % 64 == 0 and height % 64 == 0
        self.width, self.height, self.hs, self.vs, self.chroma, self.isz = width, height, hs, vs, chroma, isz
        self.mvf = np.zeros((height // 4, width // 4), ifc.MVF_DT)
        self.covered = np.zeros((height, width), bool)
        aff, gpm = [], []
        n_areas = (width // 64) * (height // 64)
        part0 = int(rng.integers(0, 64))
        for a in range(n_areas):
            x64, y64 = (a % (width // 64)) * 64, (a // (width // 64)) * 64
            for kind, dx, dy, w, h in LAYOUTS[a % len(LAYOUTS)]:
                if kind is None:
                    continue
                x, y = x64 + dx, y64 + dy
                slice_ = int(y >= height // 2)
                self.covered[y:y + h, x:x + w] = True
                if kind == AFFINE:
                    pred_flag = int(rng.choice([1, 2, 3, 3]))
                    ref_idx = rng.integers(0, 2, size=2)
                    bcw = int(rng.integers(1, 5)) if pred_flag == 3 and rng.random() < 0.4 else 0
                    base = rng.integers(-mv_range, mv_range + 1, size=(2, 2))
                    grad = rng.integers(-24, 25, size=(2, 2, 2))           # [list][d/dx, d/dy][x, y] per sub-block: motion varies inside
                    blk = self.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
                    sy_, sx_ = np.mgrid[0:h // 4, 0:w // 4]
                    for l in range(2):
                        for d in range(2):
                            blk["mv"][:, :, l, d] = base[l, d] + grad[l, 0, d] * sx_ + grad[l, 1, d] * sy_ + rng.integers(-3, 4, size=sx_.shape)
                    blk["ref_idx"] = [ref_idx[0] if pred_flag & 1 else -1, ref_idx[1] if pred_flag & 2 else -1]
                    blk["bcw_idx"], blk["pred_flag"] = bcw, pred_flag
                    prof = int(rng.integers(0, 4))
                    dmv = rng.integers(-31, 32, size=(2, 2, 16))
                    aff.append((x, y, w, h, w // 4, h // 4, prof, slice_, 0, dmv))
                else:
                    mvs = []
                    for _ in range(2):
                        m = np.zeros((), ifc.MVF_DT)
                        lx = int(rng.integers(0, 2))
                        m["pred_flag"] = lx + 1
                        m["ref_idx"] = [-1, -1]
                        m["ref_idx"][lx] = int(rng.integers(0, 2))
                        m["mv"][lx] = rng.integers(-mv_range, mv_range + 1, size=2)
                        mvs.append(m)
                    gpm.append((x, y, w, h, (part0 + len(gpm)) % 64, slice_, mvs))
        self.aff = np.zeros(len(aff), AFFINE_CU_DT)
        first = 0
        for i, (x, y, w, h, nsx, nsy, prof, sl, _, dmv) in enumerate(aff):
            r = self.aff[i]
            r["x0"], r["y0"], r["cb_width"], r["cb_height"], r["num_sb_x"], r["num_sb_y"] = x, y, w, h, nsx, nsy
            r["prof_flags"], r["slice"], r["first_job"], r["diff_mv"] = prof, sl, first, dmv
            first += nsx * nsy
        self.n_aff_jobs = first
        self.gpm = np.zeros(len(gpm), GPM_CU_DT)
        first = 0
        for i, (x, y, w, h, part, sl, mvs) in enumerate(gpm):
            r = self.gpm[i]
            r["x0"], r["y0"], r["cb_width"], r["cb_height"], r["partition_idx"], r["slice"], r["first_job"] = x, y, w, h, part, sl, first
            self.gpm.view(np.uint8).reshape(-1, GPM_CU_DT.itemsize)[i, 16:64] = np.frombuffer(mvs[0].tobytes() + mvs[1].tobytes(), np.uint8)
            first += len(gpm_tiles(w, h, self.hs, self.vs, self.chroma))
        self.n_gpm_jobs = first
        # slice 0: default weighting, LMCS on; slice 1: explicit weighted bi- and uni-prediction, no LMCS (as inter_frame_cases.py)
        self.slices = (abi.InterSlice * 2)()
        self.slices[0].lmcs_used = 1
        s1 = self.slices[1]
        s1.weighted_pred, s1.weighted_bipred = 0, 1
        s1.log2_denom[0], s1.log2_denom[1] = 6, 5
        for l in range(2):
            for c in range(3):
                for r in range(16):
                    s1.weight[l][c][r] = int(rng.integers(-32, 96))
                    s1.offset[l][c][r] = int(rng.integers(-20, 21))

    # ---- descriptors
    def pic(self, dst_ptrs, dst_strides, mvf_ptr, refs_ptr, slices_ptr, lut_ptr):
        f = abi.InterFrame()
        for c in range(3):
            f.dst[c], f.dst_stride[c] = dst_ptrs[c], dst_strides[c]
        f.mvf, f.refs, f.slices, f.lmcs_fwd_lut = mvf_ptr, refs_ptr, slices_ptr, lut_ptr
        f.mvf_stride, f.width, f.height = self.width // 4, self.width, self.height
        f.hs, f.vs, f.chroma_format_idc, f.pixel_shift = self.hs, self.vs, int(self.chroma), int(self.isz == 2)
        return f

    def n_aff_chroma_jobs(self):
        return 2 * (self.n_aff_jobs >> (self.hs + self.vs)) if self.chroma else 0

    # ---- the reference's walks
    def weights(self, sl, m, c):
        """derive_weight (dmvr_flag 0, no CIIP) / derive_weight_uni, vvc_inter.c:129-177: (weight_flag, denom, w0, w1, o0, o1)."""
        s = self.slices[sl]
        pf, ref_idx, bcw = int(m["pred_flag"]), m["ref_idx"], int(m["bcw_idx"])
        if pf == 3:
            if not (s.weighted_pred or s.weighted_bipred or bcw):
                return 0, 0, 0, 0, 0, 0
            if bcw:
                w1 = (4, 5, 3, 10, -2)[bcw]                               # bcw_w_lut, vvc_inter.c:29
                return 1, 2, 8 - w1, w1, 0, 0
            r0, r1 = int(ref_idx[0]), int(ref_idx[1])
            return 1, s.log2_denom[c > 0], s.weight[0][c][r0], s.weight[1][c][r1], s.offset[0][c][r0], s.offset[1][c][r1]
        if not (s.weighted_pred or s.weighted_bipred):
            return 0, 0, 0, 0, 0, 0
        lx = pf - 1
        r = int(ref_idx[lx])
        return 1, s.log2_denom[c > 0], s.weight[lx][c][r], 0, s.offset[lx][c][r], 0

    def expect_affine(self, plane, ref, cu_addr, lut):
        """pred_affine_blk (vvc_inter.c:828-873) with plane(c) -> (address, stride) of the current picture, ref(l, r, c) -> (address,
        stride), cu_addr(u) -> address of record u, lut = forward map address: (luma jobs, chroma jobs Cb / Cr interleaved)."""
        jl = np.zeros(self.n_aff_jobs, AFFINE_JOB_DT)
        jc = np.zeros(self.n_aff_chroma_jobs(), BIPRED_JOB_DT)
        hs, vs = self.hs, self.vs
        for u, cu in enumerate(self.aff):
            x0, y0, nsx, nsy, sl = int(cu["x0"]), int(cu["y0"]), int(cu["num_sb_x"]), int(cu["num_sb_y"]), int(cu["slice"])
            first = int(cu["first_job"])
            for sby in range(nsy):                                          # :842-843
                for sbx in range(nsx):
                    x, y = x0 + 4 * sbx, y0 + 4 * sby                       # :844-845, sbw = sbh = 4
                    mv = self.mvf[y >> 2, x >> 2]                           # :848 ff_vvc_get_mvf
                    j = jl[first + sby * nsx + sbx]
                    base, stride = plane(0)
                    j["dst"], j["dst_stride"] = base + y * stride + x * self.isz, stride
                    for l in range(2):                                      # :850 pred_get_refs
                        if int(mv["pred_flag"]) & (1 << l):
                            j[f"ref{l}"], j[f"ref{l}_stride"] = ref(l, int(mv["ref_idx"][l]), 0)
                            j["mv"][2 * l:2 * l + 2] = mv["mv"][l]
                    j["diff_mv"] = cu_addr(u) + 16                          # pu->diff_mv_x / _y (:856-857)
                    j["x"], j["y"], j["pic_w"], j["pic_h"] = x, y, self.width, self.height
                    j["weight_flag"], j["denom"], j["w0"], j["w1"], j["o0"], j["o1"] = self.weights(sl, mv, 0)     # luma_prof_uni / _bi
                    j["pred_flag"], j["prof0"], j["prof1"] = mv["pred_flag"], int(cu["prof_flags"]) & 1, int(cu["prof_flags"]) >> 1 & 1
                    j["lmcs_lut"] = lut if self.slices[sl].lmcs_used else 0  # predict_inter :888-891
                    if not self.chroma or sbx % (1 << hs) or sby % (1 << vs):   # :863
                        continue
                    mv2 = self.mvf[(y + vs * 4) >> 2, (x + hs * 4) >> 2]   # derive_affine_mvc (:813-826)
                    mvc = np.zeros((), ifc.MVF_DT)                          # a copy: np.array(mv) would alias the table
                    mvc[()] = mv
                    mvc["mv"] = round_half(mv["mv"].astype(np.int64) + mv2["mv"])
                    k = (first >> (hs + vs)) + (sby >> vs) * (nsx >> hs) + (sbx >> hs)
                    for c in (1, 2):                                        # pred_regular_chroma (:583-640), 4x4 chroma samples
                        b = jc[2 * k + c - 1]
                        xc, yc = x >> hs, y >> vs
                        base, stride = plane(c)
                        b["dst"], b["dst_stride"] = base + yc * stride + xc * self.isz, stride
                        for l in range(2):
                            if int(mvc["pred_flag"]) & (1 << l):
                                b[f"ref{l}"], b[f"ref{l}_stride"] = ref(l, int(mvc["ref_idx"][l]), c)
                                b["mv"][2 * l:2 * l + 2] = mvc["mv"][l]
                        b["x"], b["y"], b["w"], b["h"] = xc, yc, 4, 4
                        b["pic_w"], b["pic_h"] = self.width >> hs, self.height >> vs
                        b["chroma"], b["hs"], b["vs"] = 1, hs, vs
                        b["weight_flag"], b["denom"], b["w0"], b["w1"], b["o0"], b["o1"] = self.weights(sl, mvc, c)
                        b["pred_flag"] = mvc["pred_flag"]
        return jl, jc

    def expect_gpm(self, plane, ref, lut, masks, tables):
        """pred_gpm_blk (vvc_inter.c:466-527) with the maps of expect_affine; `masks` = address of ff_vvc_gpm_weights[6][112 * 112] (uint8),
        `tables` = the fixture's other GPM tables.  Tiles of <= 16x16 per component, in gpm_tiles order."""
        jobs = np.zeros(self.n_gpm_jobs, GPM_JOB_DT)
        for cu in self.gpm:
            x0, y0, cbw, cbh, part, sl = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height", "partition_idx", "slice"))
            angle = int(tables["ff_vvc_gpm_angle_idx"][part])                               # :472-480
            widx = int(tables["ff_vvc_gpm_angle_to_weights_idx"][angle])
            wl, hl = cbw.bit_length() - 4, cbh.bit_length() - 4
            off_x = int(tables["ff_vvc_gpm_weights_offset_x"][part, hl, wl])
            off_y = int(tables["ff_vvc_gpm_weights_offset_y"][part, hl, wl])
            mirror = int(tables["ff_vvc_gpm_angle_to_mirror"][angle])
            mvs = cu["gpm_mv"]
            for i, (c, tx, ty, tw, th) in enumerate(gpm_tiles(cbw, cbh, self.hs, self.vs, self.chroma)):
                hs, vs = (self.hs, self.vs) if c else (0, 0)
                g = jobs[int(cu["first_job"]) + i]
                j = g["base"]
                x, y = (x0 >> hs) + tx, (y0 >> vs) + ty
                base, stride = plane(c)
                j["dst"], j["dst_stride"] = base + y * stride + x * self.isz, stride
                for p in range(2):                                                           # :500-509
                    lx = int(mvs[p]["pred_flag"]) - 1
                    j[f"ref{p}"], j[f"ref{p}_stride"] = ref(lx, int(mvs[p]["ref_idx"][lx]), c)
                    j["mv"][2 * p:2 * p + 2] = mvs[p]["mv"][lx]
                j["x"], j["y"], j["w"], j["h"] = x, y, tw, th
                j["pic_w"], j["pic_h"] = self.width >> hs, self.height >> vs
                j["chroma"], j["hs"], j["vs"], j["pred_flag"] = int(c > 0), self.hs, self.vs, 3
                j["lmcs_lut"] = lut if (c == 0 and self.slices[sl].lmcs_used) else 0
                step_x, step_y = 1 << hs, 112 << vs                                         # :486-497
                if mirror == 0:
                    first = off_y * 112 + off_x
                elif mirror == 1:
                    step_x, first = -step_x, off_y * 112 + 111 - off_x
                else:
                    step_y, first = -step_y, (111 - off_y) * 112 + off_x
                g["weights"] = masks + widx * 112 * 112 + first + ty * step_y + tx * step_x
                g["step_x"], g["step_y"] = step_x, step_y
        return jobs


def ref_table(ptrs, strides):
    t = (abi.RefPic * 32)()
    for l in range(2):
        for r in range(2):
            for c in range(3):
                t[l * 16 + r].plane[c] = ptrs[l][r][c]
                t[l * 16 + r].stride[c] = strides[l][r][c]
    return t


def call(fn, bd, arr):
    """Run an oracle block function on every job of a structured array."""
    saved = fn.argtypes, fn.restype
    fn.argtypes, fn.restype = [ctypes.c_int, ctypes.c_void_p], None
    try:
        for i in range(len(arr)):
            fn(bd, arr[i:i + 1].ctypes.data)
    finally:
        fn.argtypes, fn.restype = saved

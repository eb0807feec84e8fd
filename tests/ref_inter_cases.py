"""Pictures, frames, host runs and digests for the inter prediction passes pinned against the reference's own callers
(oracle/ref_shim_inter.c: ff_vvc_predict_inter and ff_vvc_predict_ciip on real contexts): regular pictures R0-R7, affine pictures A0-A3,
geometric-partition pictures G0-G2, CIIP pictures I0-I4 (the five of ciip_frame_cases, whose slices are CTU-aligned), the mixed picture M0
(regular, affine and GPM units together) and the freshly drawn pictures of the sweep.  Used by tests/test_ref_inter_cpu.py,
tests/test_ref_inter_gpu.py and tools/gen_golden.py; tests/golden/ref_inter.json holds the reference's digests.

Every picture is deterministic.  A CTU is split at random into power-of-two units (4x8 .. 128x128, cut to fit pictures whose size is a
multiple of 8 but not of the CTU), some of which are left out so that the sentinel the planes start with has to survive; slices are
CTU-aligned (the reference keeps one SliceContext per CTU): slice 0 default weights + LMCS, slice 1 B-typed with explicit weights and no
LMCS, slice 2 P-typed with explicit weights + LMCS.  Content is bipred_cases.smooth_picture / shifted, so that DMVR has something to find;
a share of the DMVR units has list-1 motion aimed at a chosen refinement (exact match, fractional offset, offset on the border of the
search array, offset of more than a sample), and a share of the units on the picture's edge has motion that leaves it there.

What stays out, because the stage drivers' header excludes it: CIIP units in the regular list (vvc355_inter_frame_pass would predict them
onto the picture; ff_vvc_predict_inter skips them, so the shim refuses them).  The GPM pictures leave out 4:0:0.  Units 4 wide are
uni-predicted (chroma 2 wide at 4:2:0), as the standard has them.  ref_idx stays below 15: the reference's weight table holds 15 entries.

Sensitivity, checked on the CPU with the oracle as stand-in (one perturbation of the oracle's restatement at a time, listed pictures that then
no longer hash to the reference's digests):
  refined instead of unrefined window in emulated_edge_dmvr   R0 R1 R2 R3 R4 R5 R6 R7 M0 (planes)
  `!dmvr_flag` dropped in derive_weight                       R0 R1 R2 R3 R5 (planes), R4 R6 (chroma planes)
  step_x's sign swapped for mirror type 1                     G0 G1 G2 M0 (planes)
  forward map applied to CIIP chroma                          I0 I1 I2 I4 (scratch; I0 I2 I4 also the chroma planes of 2-wide blocks)
  derive_affine_mvc rounded toward zero                       none, and none can: with a shift of one, ff_vvc_round_mv's
      (v + 1 - (v >= 0)) >> 1 IS v / 2 rounded toward zero (v >= 0: v >> 1; v < 0: (v + 1) >> 1), so that restatement computes what the
      reference computes.  The roundings that do differ are each caught by A0 A2 M0 (chroma planes; A1 is 4:4:4, where the sum is even, A3
      4:0:0): toward minus infinity (v >> 1), half up ((v + 1) >> 1), half away from zero.  test_ref_inter_cpu.py counts the odd
      negative and odd positive sums these need.
"""
import ctypes
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np

import affine_gpm_cases as agc
import bipred_cases as bc
import ciip_frame_cases as cc
import inter_frame_cases as ifc
from ffvvc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_inter.json")
GPM_TABLES = np.load(os.path.join(ROOT, "tests", "golden", "gpm_tables.npz"))
GPM_MASKS = np.ascontiguousarray(GPM_TABLES["ff_vvc_gpm_weights"])
SEED = 0x1E7E4000
FMT = cc.FMT                                   # chroma_format_idc -> (hs, vs)
BCW_W1 = (4, 5, 3, 10, -2)                     # bcw_w_lut

# name -> bit depth, chroma_format_idc, CTU log2, (width, height), unit kinds; `whole`: CTUs taken as ONE bi-predicted unit with the given
# flags (d = DMVR, b = BDOF; affine pictures: any string), `mv_range` in 1/16 sample
_LISTED = {
    "R0": dict(bd=10, idc=1, ctb_log2=6, size=(256, 192), kinds="R"),
    "R1": dict(bd=8, idc=3, ctb_log2=5, size=(200, 136), kinds="R"),
    "R2": dict(bd=12, idc=2, ctb_log2=7, size=(256, 192), kinds="R", whole={0: "db", 1: "", 2: "d"}),
    "R3": dict(bd=10, idc=0, ctb_log2=6, size=(200, 136), kinds="R"),
    "R4": dict(bd=8, idc=1, ctb_log2=7, size=(248, 184), kinds="R", mv_range=300 * 16),
    "R5": dict(bd=10, idc=2, ctb_log2=5, size=(136, 184), kinds="R"),
    "R6": dict(bd=12, idc=3, ctb_log2=6, size=(192, 128), kinds="R"),
    "R7": dict(bd=10, idc=1, ctb_log2=7, size=(256, 192), kinds="R", whole={0: "b", 2: ""}),
    "A0": dict(bd=10, idc=1, ctb_log2=6, size=(256, 192), kinds="A"),
    "A1": dict(bd=8, idc=3, ctb_log2=5, size=(200, 136), kinds="A"),
    "A2": dict(bd=12, idc=2, ctb_log2=7, size=(256, 192), kinds="A", whole={0: "a"}),
    "A3": dict(bd=10, idc=0, ctb_log2=6, size=(136, 184), kinds="A"),
    "G0": dict(bd=10, idc=1, ctb_log2=6, size=(256, 192), kinds="G"),
    "G1": dict(bd=8, idc=3, ctb_log2=5, size=(200, 136), kinds="G"),
    "G2": dict(bd=12, idc=2, ctb_log2=7, size=(248, 184), kinds="G"),
    "M0": dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), kinds="RAG"),
}
REGULAR = [n for n in _LISTED if n[0] == "R"]
AFFINE = [n for n in _LISTED if n[0] == "A"]
GPM = [n for n in _LISTED if n[0] == "G"]
CIIP = [f"I{i}" for i in range(len(cc.CASES))]
MIXED = "M0"
GPM_SHAPES = sorted((w, h) for w in (8, 16, 32, 64) for h in (8, 16, 32, 64) if w < 8 * h and h < 8 * w)

# DMVR refinements a unit's list-1 motion is aimed at, in 1/32 sample (the bilinear search sees list 0 displaced by +d, list 1 by -d)
_AIMS = [(0, 0), (10, -20), (64, 32), (-46, 16), (32, -64), (-64, -64), (24, 40), (-32, 8)]


def px(bd):
    return np.uint8 if bd == 8 else np.uint16


# ---------------------------------------------------------------------------------------------------------------- drawing a picture

def _split(rng, x, y, w, h, W, H, min_side, out):
    """Leaves of a random binary / quad split of the block, cut to the picture: power-of-two sides, 4-wide only as 4x8 / 4x16 (and transposed)."""
    if x >= W or y >= H:
        return
    over_x, over_y = x + w > W, y + h > H
    ok = lambda a, b: min(a, b) >= min_side and (min(a, b) > 4 or max(a, b) in (8, 16))          # noqa: E731
    opts = []
    if over_x or over_y:
        opts = ["q"] if over_x and over_y and w == h else ["v"] if over_x and (not over_y or w >= h) else ["h"]
    else:
        stop = {128: 0.3, 64: 0.3, 32: 0.35, 16: 0.45, 8: 0.7}.get(max(w, h), 1.0)
        if rng.random() >= stop:
            opts = [o for o, good in (("q", w == h and ok(w // 2, h // 2)), ("v", ok(w // 2, h)), ("h", ok(w, h // 2))) if good]
    if not opts:
        out.append((x, y, w, h))
        return
    o = opts[int(rng.integers(0, len(opts)))]
    if o == "q":
        for dy in (0, h // 2):
            for dx in (0, w // 2):
                _split(rng, x + dx, y + dy, w // 2, h // 2, W, H, min_side, out)
    elif o == "v":
        for dx in (0, w // 2):
            _split(rng, x + dx, y, w // 2, h, W, H, min_side, out)
    else:
        for dy in (0, h // 2):
            _split(rng, x, y + dy, w, h // 2, W, H, min_side, out)


def make_slices(rng):
    slices = (abi.InterSlice * 3)()
    slices[0].lmcs_used = 1
    slices[1].weighted_bipred = 1
    slices[2].weighted_pred, slices[2].lmcs_used = 1, 1
    for s in (slices[1], slices[2]):
        s.log2_denom[0], s.log2_denom[1] = 6, 5
        for l in range(2):
            for c in range(3):
                for r in range(16):
                    s.weight[l][c][r] = int(rng.integers(-32, 96))
                    s.offset[l][c][r] = int(rng.integers(-20, 21))
    return slices


def ref_shift(l, r):
    """(dx, dy) of reference picture r of list l against the common base picture, luma samples: ref[y, x] = base[y + dy, x + dx]."""
    return (2 * l - 1) * (r + 1), (1 - 2 * l) * (r + 2)


class Picture(agc.AffineGpmWork):
    """One picture of any of the three unit kinds.  agc.AffineGpmWork's expect_affine / expect_gpm / weights (the numpy walks the GPU parity
    tests use) run on it unchanged: they read width, height, hs, vs, chroma, isz, mvf, aff, gpm, slices and the job counts."""

    def __init__(self, name, rng, bd, idc, ctb_log2, size, kinds, whole=None, mv_range=20 * 16, hole=0.1, content=None, layout=None):
        """content(self) -> refs[list][ref_idx][component], called last, replaces the smooth reference pictures; layout(self) -> (pus, aff,
        gpm) in the forms of _regular / _affine / _gpm places the units by hand instead of the random split (it fills self.mvf, self.units
        and self.covered, and may replace self.slices and self.ctu_slice).  Both default to None: the listed pictures draw what they drew."""
        self.name, self.bd, self.idc, self.ctb_log2, self.kinds = name, bd, idc, ctb_log2, kinds
        self.width, self.height = size
        assert self.width % 8 == 0 and self.height % 8 == 0 and self.width <= 264 and self.height <= 192
        assert "G" not in kinds or idc, "GPM pictures leave out 4:0:0"
        self.hs, self.vs = FMT[idc]
        self.chroma, self.isz = idc != 0, 1 if bd == 8 else 2
        self.n_comp = 3 if self.chroma else 1
        self.dims = [(self.width, self.height)] + [(self.width >> self.hs, self.height >> self.vs)] * 2
        self.sentinel = (1 << bd) // 3
        W, H, ctb = self.width, self.height, 1 << ctb_log2
        self.ncx, self.ncy = (W + ctb - 1) // ctb, (H + ctb - 1) // ctb
        n_ctb = self.ncx * self.ncy
        self.ctu_slice = [min(2, rs * 3 // n_ctb) if n_ctb >= 3 else rs % 3 for rs in range(n_ctb)]
        self.slices = make_slices(rng)
        self.mvf = np.zeros((H // 4, W // 4), ifc.MVF_DT)
        self.covered = np.zeros((H, W), bool)
        self.units = []                            # (kind, x, y, w, h) of every unit, for messages
        if content is None:
            base = [bc.smooth_picture(rng, ph, pw, bd) for (pw, ph) in self.dims]
            self.refs = [[[bc.shifted(base[c], ref_shift(l, r)[0] >> (self.hs if c else 0), ref_shift(l, r)[1] >> (self.vs if c else 0)) for c in range(3)]
                          for r in range(2)] for l in range(2)]
        self.lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(px(bd))          # fc->ps.lmcs.fwd_lut
        pus, aff, gpm = [], [], []
        self._part = int(rng.integers(0, 64))
        min_side = 4 if "R" in kinds else 8
        if layout is not None:
            pus, aff, gpm = layout(self)
        else:
            for rs in range(n_ctb):
                x0, y0, sl = (rs % self.ncx) * ctb, (rs // self.ncx) * ctb, self.ctu_slice[rs]
                leaves, forced = [], None
                if whole and rs in whole:
                    leaves, forced = [(x0, y0, min(ctb, W - x0), min(ctb, H - y0))], whole[rs]
                else:
                    _split(rng, x0, y0, ctb, ctb, W, H, min_side, leaves)
                for (x, y, w, h) in leaves:
                    fits = {"R": True, "A": w >= 8 and h >= 8, "G": (w, h) in GPM_SHAPES}
                    opts = [k for k in kinds if fits[k]]
                    if not opts or (forced is None and rng.random() < hole):
                        continue
                    kind = opts[int(rng.integers(0, len(opts)))]
                    self.covered[y:y + h, x:x + w] = True
                    self.units.append((kind, x, y, w, h))
                    if kind == "R":
                        pus.append(self._regular(rng, x, y, w, h, sl, mv_range, forced))
                    elif kind == "A":
                        aff.append(self._affine(rng, x, y, w, h, sl, mv_range))
                    else:
                        gpm.append(self._gpm(rng, x, y, w, h, sl, mv_range, len(gpm)))
        self._finish(pus, aff, gpm)
        if content is not None:
            self.refs = content(self)
        # the reference's PredWeightTable holds 15 entries per list: ref_idx 15 of an explicitly weighted slice would read past it
        assert int(self.mvf["ref_idx"].max()) < 15 and all(int(m["ref_idx"].max()) < 15 for cu in self.gpm for m in cu["gpm_mv"].view(ifc.MVF_DT))

    # ---- the three kinds of unit
    def _edge_aim(self, rng, x, y, w, h, mv, used):
        """Motion that leaves the picture where the unit touches its edge, for half of those units."""
        sx = -1 if x == 0 else 1 if x + w == self.width else 0
        sy = -1 if y == 0 else 1 if y + h == self.height else 0
        if (sx or sy) and rng.random() < 0.5:
            for l in used:
                if sx:
                    mv[l, 0] = sx * int(rng.integers(6 * 16, 30 * 16))
                if sy:
                    mv[l, 1] = sy * int(rng.integers(6 * 16, 30 * 16))

    def _regular(self, rng, x, y, w, h, sl, mv_range, forced):
        small = min(w, h) == 4
        pred_flag = 3 if forced is not None else int(rng.choice([1, 2] if small else [1, 2, 3, 3, 3]))
        bi = pred_flag == 3
        big = w >= 8 and h >= 8 and w * h >= 128
        sub_merge = forced is None and w >= 8 and h >= 8 and max(w, h) >= 16 and rng.random() < 0.15          # sub-block merge, 8x8 sub-blocks
        dmvr = int(bi and big and not sub_merge and rng.random() < 0.5) if forced is None else int("d" in forced)
        bdof = int(bi and big and not sub_merge and rng.random() < 0.5) if forced is None else int("b" in forced)
        bcw = int(rng.integers(1, 5)) if (bi and not dmvr and not bdof and not sub_merge and rng.random() < 0.35) else 0
        hpel = int(rng.random() < 0.2)
        if sub_merge:
            nsx, nsy = w // 8, h // 8
        elif dmvr or bdof:
            nsx, nsy = max(1, w // 16), max(1, h // 16)
        else:
            nsx, nsy = 1, 1
        base = rng.integers(-mv_range, mv_range + 1, size=(2, 2))
        if hpel:
            base = base // 8 * 8                    # half-sample positions
        ref_idx = rng.integers(0, 2, size=2)
        self._edge_aim(rng, x, y, w, h, base, [l for l in range(2) if pred_flag & (1 << l)])
        if dmvr and rng.random() < 0.75:
            # list 1 against list 0 so that the two predictions match at the refinement d (the reference pictures are shifts of one picture)
            d = _AIMS[int(rng.integers(0, len(_AIMS)))]
            s0, s1 = ref_shift(0, int(ref_idx[0])), ref_shift(1, int(ref_idx[1]))
            base[1] = [base[0, k] + d[k] - 16 * (s1[k] - s0[k]) for k in range(2)]
        sbw, sbh = w // nsx, h // nsy
        for sy in range(nsy):
            for sx in range(nsx):
                pf = int(rng.choice([1, 2, 3])) if sub_merge and rng.random() < 0.3 else pred_flag       # sub-block motion may change direction too
                mv = base + (rng.integers(-6, 7, size=(2, 2)) * (8 if hpel else 1) if sub_merge else 0)
                blk = self.mvf[(y + sy * sbh) // 4:(y + (sy + 1) * sbh) // 4, (x + sx * sbw) // 4:(x + (sx + 1) * sbw) // 4]
                blk["mv"] = mv
                blk["ref_idx"] = [ref_idx[0] if pf & 1 else -1, ref_idx[1] if pf & 2 else -1]
                blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"] = hpel, bcw, pf
        return (x, y, w, h, nsx, nsy, dmvr, bdof, 0, hpel, sl, 0, 0)

    def _affine(self, rng, x, y, w, h, sl, mv_range):
        pred_flag = int(rng.choice([1, 2, 3, 3]))
        ref_idx = rng.integers(0, 2, size=2)
        bcw = int(rng.integers(1, 5)) if pred_flag == 3 and rng.random() < 0.4 else 0
        base = rng.integers(-mv_range, mv_range + 1, size=(2, 2))
        self._edge_aim(rng, x, y, w, h, base, [l for l in range(2) if pred_flag & (1 << l)])
        grad = rng.integers(-24, 25, size=(2, 2, 2))           # [list][d/dx, d/dy][x, y] per sub-block: motion varies inside
        blk = self.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
        sy_, sx_ = np.mgrid[0:h // 4, 0:w // 4]
        for l in range(2):
            for d in range(2):
                blk["mv"][:, :, l, d] = base[l, d] + grad[l, 0, d] * sx_ + grad[l, 1, d] * sy_ + rng.integers(-3, 4, size=sx_.shape)
        blk["ref_idx"] = [ref_idx[0] if pred_flag & 1 else -1, ref_idx[1] if pred_flag & 2 else -1]
        blk["bcw_idx"], blk["pred_flag"] = bcw, pred_flag
        return (x, y, w, h, int(rng.integers(0, 4)), sl, rng.integers(-31, 32, size=(2, 2, 16)))

    def _gpm(self, rng, x, y, w, h, sl, mv_range, k):
        mvs = []
        for _ in range(2):
            m = np.zeros((), ifc.MVF_DT)
            lx = int(rng.integers(0, 2))
            m["pred_flag"] = lx + 1
            m["ref_idx"] = [-1, -1]
            m["ref_idx"][lx] = int(rng.integers(0, 2))
            mv = rng.integers(-mv_range, mv_range + 1, size=(2, 2))
            self._edge_aim(rng, x, y, w, h, mv, [lx])
            m["mv"][lx] = mv[lx]
            mvs.append(m)
        return (x, y, w, h, (self._part + k) % 64, sl, mvs)

    def _finish(self, pus, aff, gpm):
        self.pus = np.array(pus, dtype=ifc.PU_DT) if pus else np.zeros(0, ifc.PU_DT)
        counts = np.array([ifc.n_jobs_of(p["cb_width"], p["cb_height"], p["num_sb_x"], p["num_sb_y"]) for p in self.pus], np.int64)
        self.pus["first_job"] = np.concatenate(([0], np.cumsum(counts)[:-1])) if len(pus) else []
        self.n_jobs = int(counts.sum())
        self.aff = np.zeros(len(aff), agc.AFFINE_CU_DT)
        first = 0
        for i, (x, y, w, h, prof, sl, dmv) in enumerate(aff):
            r = self.aff[i]
            r["x0"], r["y0"], r["cb_width"], r["cb_height"], r["num_sb_x"], r["num_sb_y"] = x, y, w, h, w // 4, h // 4
            r["prof_flags"], r["slice"], r["first_job"], r["diff_mv"] = prof, sl, first, dmv
            first += (w // 4) * (h // 4)
        self.n_aff_jobs = first
        self.gpm = np.zeros(len(gpm), agc.GPM_CU_DT)
        first = 0
        for i, (x, y, w, h, part, sl, mvs) in enumerate(gpm):
            r = self.gpm[i]
            r["x0"], r["y0"], r["cb_width"], r["cb_height"], r["partition_idx"], r["slice"], r["first_job"] = x, y, w, h, part, sl, first
            self.gpm.view(np.uint8).reshape(-1, agc.GPM_CU_DT.itemsize)[i, 16:64] = np.frombuffer(mvs[0].tobytes() + mvs[1].tobytes(), np.uint8)
            first += len(agc.gpm_tiles(w, h, self.hs, self.vs, self.chroma))
        self.n_gpm_jobs = first

    # ---- descriptors
    def frame(self, dst_ptrs, dst_strides, mvf_ptr, refs_ptr, slices_ptr, lut_ptr, pus_ptr=0, jl_ptr=0, jc_ptr=0, rec_ptr=0, dmvr_ptr=0):
        f = self.pic(dst_ptrs, dst_strides, mvf_ptr, refs_ptr, slices_ptr, lut_ptr)
        f.chroma_format_idc = self.idc
        f.pus, f.jobs_luma, f.jobs_chroma, f.records, f.dmvr_mvf = pus_ptr, jl_ptr, jc_ptr, rec_ptr, dmvr_ptr
        f.n_pus, f.n_jobs = len(self.pus), self.n_jobs
        return f

    def unit_at(self, c, row, col):
        """The unit that covers sample (row, col) of component c, or None."""
        x, y = col << (self.hs if c else 0), row << (self.vs if c else 0)
        for u in self.units:
            if u[1] <= x < u[1] + u[3] and u[2] <= y < u[2] + u[4]:
                return u
        return None


_pictures = {}


def picture(name):
    """A listed picture (R*, A*, G*, M0), made once per process; nobody writes to it."""
    if name not in _pictures:
        c = _LISTED[name]
        _pictures[name] = Picture(name, np.random.default_rng(SEED + sum(map(ord, name)) * 7 + int(name[1:])), c["bd"], c["idc"], c["ctb_log2"], c["size"],
                                  c["kinds"], whole=c.get("whole"), mv_range=c.get("mv_range", 20 * 16))
    return _pictures[name]


def sweep_picture(kind, k):
    """Picture k of the sweep of one unit kind ("R", "A", "G"): free size up to 264x136 in multiples of 8, format, depth, CTU size, unit mix."""
    rng = np.random.default_rng(SEED + 10000 * (1 + "RAG".index(kind)) + k)
    idc = int(rng.integers(1 if kind == "G" else 0, 4))
    size = (8 * int(rng.integers(2, 34)), 8 * int(rng.integers(2, 18)))
    return Picture(f"sweep-{kind}-{k}", rng, int(rng.choice([8, 10, 12])), idc, int(rng.integers(5, 8)), size, kind,
                   mv_range=int(rng.choice([6 * 16, 20 * 16, 300 * 16])), hole=float(rng.choice([0.0, 0.1, 0.3])))


# ---------------------------------------------------------------------------------------------------------------- CIIP pictures

def _ciip_inputs(p, name, seed):
    dims, refs, lut = cc.pictures(np.random.default_rng(seed), p, p.bd)
    return SimpleNamespace(name=name, p=p, bd=p.bd, dims=dims, refs=refs, lut=lut, sentinel=(1 << p.bd) // 3, n_comp=3 if p.chroma else 1)


_ciip = {}


def ciip_picture(name):
    """I0-I4: ciip_frame_cases.case_picture(i) with reference pictures of its own.  Their two slices split after the first CTU row."""
    if name not in _ciip:
        i = int(name[1:])
        _ciip[name] = _ciip_inputs(cc.case_picture(i), name, SEED + 500 + i)
    return _ciip[name]


def sweep_ciip(k):
    """A freshly drawn CIIP picture with ciip_frame_cases' premises: units of 4..64 a side and at least 64 samples on a background of 8x8
    blocks that are intra or inter at random, two slices split after the first CTU row, tiles at random, the command array with its oddities."""
    rng = np.random.default_rng(SEED + 50000 + k)
    bd, idc, ctb_log2 = int(rng.choice([8, 10, 12])), int(rng.integers(0, 4)), int(rng.integers(5, 8))
    W, H = 8 * int(rng.integers(2, 34)), 8 * int(rng.integers(2, 18))
    p = cc.CiipPicture(W, H, ctb_log2, idc, 1 if bd == 8 else 2)
    p.bd, p.mv_range = bd, int(rng.choice([6 * 16, 20 * 16, 300 * 16]))
    p.slice_idx[:] = (np.arange(p.ncx * p.ncy) // p.ncx > 0).astype(np.int16)
    if rng.random() < 0.5:
        cx, cy = int(rng.integers(0, p.ncx)), int(rng.integers(0, p.ncy))
        p.col_bd = np.array([0 if x < cx else cx for x in range(p.ncx)] + [p.ncx], np.int16)
        p.row_bd = np.array([0 if y < cy else cy for y in range(p.ncy)] + [p.ncy], np.int16)
    p.slices = cc.make_slices(rng)
    cc.fill_background(rng, p.mvf)
    ctb, units = 1 << ctb_log2, []
    for rs in range(p.ncx * p.ncy):
        leaves = []
        _split(rng, (rs % p.ncx) * ctb, (rs // p.ncx) * ctb, ctb, ctb, W, H, 4, leaves)
        for (x, y, w, h) in leaves:
            if w > 64 or h > 64 or w * h < 64 or rng.random() < 0.4:
                continue
            hpel = int(rng.random() < 0.2)
            pf, ref_idx, bcw, mv = cc.random_motion(rng, p.mv_range, hpel)
            blk = p.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
            blk["mv"], blk["ref_idx"], blk["hpel_if_idx"], blk["bcw_idx"], blk["pred_flag"], blk["ciip_flag"] = mv, ref_idx, hpel, bcw, pf, 1
            units.append((x, y, w, h, hpel, int(p.slice_idx[rs])))
    p.set_records(rng, units)
    cc.build_commands(rng, p)
    return _ciip_inputs(p, f"sweep-I-{k}", SEED + 60000 + k)


def ciip_weights(cp, unit_weight):
    """int32 [unit][3]: the intra weight per blended component (0 where the reference does not blend: 4:0:0, chroma 2 wide)."""
    p = cp.p
    out = np.zeros((len(p.cus), 3), np.int32)
    for u, cu in enumerate(p.cus):
        out[u, 0] = unit_weight[u]
        if p.chroma and (int(cu["cb_width"]) >> p.hs) > 2:
            out[u, 1:] = unit_weight[u]
    return out


def ciip_joint(cp, weights):
    """The .joint byte of every command after the builder's patch, with the intra weights taken from `weights` ([unit][3]): which commands are
    patched is cc.expect_cmds' identity check (structure only), what is patched in comes from the side that ran."""
    p = cp.p
    out = p.cmds["joint"].copy()
    for u, cu in enumerate(p.cus):
        x0, y0, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
        for c in range(cp.n_comp):
            idx = int(cu["cmd"][c])
            if (c and (w >> p.hs) <= 2) or idx >= len(out):
                continue
            k = p.cmds[idx]
            if k["kind"] == abi.RECON_CIIP and k["c_idx"] == c and (int(k["x0"]), int(k["y0"]), int(k["w"]), int(k["h"])) == (x0, y0, w, h):
                out[idx] = weights[u, c]
    return out


# ---------------------------------------------------------------------------------------------------------------- host runs

def _proto(lib, name, *args):
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = list(args), (ctypes.c_int if name.startswith("ref_") else None)
    return fn


class _Host:
    """The host-side twin of a picture's device state: packed planes, tables and the frame over them."""

    def __init__(self, pic, planes=None):
        self.pic = pic
        dt = px(pic.bd)
        self.planes = planes if planes is not None else [np.full((ph, pw), pic.sentinel, dt) for (pw, ph) in pic.dims[:pic.n_comp]]
        self.mvf, self.dmvr = pic.mvf.copy(), pic.mvf.copy()       # tab_dmvr_mvf as the parser leaves it: a copy of the motion field
        self.refs = [[[a.copy() for a in r] for r in l] for l in pic.refs]
        self.lut, self.pus, self.aff, self.gpm = pic.lut.copy(), pic.pus.copy(), pic.aff.copy(), pic.gpm.copy()
        self.slices = type(pic.slices).from_buffer_copy(pic.slices)
        self.reft = agc.ref_table([[[a.ctypes.data for a in r] for r in l] for l in self.refs], [[[a.strides[0] for a in r] for r in l] for l in self.refs])
        self.jl, self.jc = np.zeros(pic.n_jobs, agc.BIPRED_JOB_DT), np.zeros(2 * pic.n_jobs, agc.BIPRED_JOB_DT)
        self.rec = np.zeros((pic.n_jobs, 8), np.int32)
        ptrs = [p.ctypes.data for p in self.planes] + [0] * (3 - len(self.planes))
        strides = [p.strides[0] for p in self.planes] + [0] * (3 - len(self.planes))
        self.f = pic.frame(ptrs, strides, self.mvf.ctypes.data, ctypes.addressof(self.reft), ctypes.addressof(self.slices), self.lut.ctypes.data,
                           self.pus.ctypes.data, self.jl.ctypes.data, self.jc.ctypes.data, self.rec.ctypes.data, self.dmvr.ctypes.data)

    def plane(self, c):
        return self.planes[c].ctypes.data, self.planes[c].strides[0]

    def ref(self, l, r, c):
        return self.refs[l][r][c].ctypes.data, self.refs[l][r][c].strides[0]

    def untouched(self, side):
        pic = self.pic
        for n in ("mvf", "lut", "pus", "aff", "gpm"):
            assert np.array_equal(getattr(self, n).view(np.uint8), getattr(pic, n).view(np.uint8)), f"{pic.name}: {side} wrote to the input {n}"
        assert bytes(self.slices) == bytes(pic.slices), f"{pic.name}: {side} wrote to the slice table"
        for l in range(2):
            for r in range(2):
                for c in range(3):
                    assert np.array_equal(self.refs[l][r][c], pic.refs[l][r][c]), f"{pic.name}: {side} wrote to a reference picture"


def run_picture(lib, side, pic, stages="RAG"):
    """The picture's units of the given kinds, in this order on the same sentinel-filled planes, on the host: by the reference ("ref":
    ref_inter_picture / ref_affine_picture / ref_gpm_picture) or by the oracle ("orc": orc_inter_frame_pass; the job arrays of
    expect_affine / expect_gpm through orc_affine_block / orc_bipred_block / orc_gpm_block).  Returns planes, dmvr (tab_dmvr_mvf) and, from
    the oracle, the regular job arrays and records (jl, jc, rec) and the affine / GPM job arrays (aff_jl, aff_jc, gpm_jobs)."""
    h = _Host(pic)
    out = SimpleNamespace(planes=h.planes, dmvr=h.dmvr, jl=h.jl, jc=h.jc, rec=h.rec, aff_jl=None, aff_jc=None, gpm_jobs=None)
    for kind in stages:
        if kind not in pic.kinds:
            continue
        if side == "ref":
            if kind == "R":
                err = _proto(lib, "ref_inter_picture", ctypes.c_int, ctypes.POINTER(abi.InterFrame), ctypes.c_int)(pic.bd, ctypes.byref(h.f), pic.ctb_log2)
            elif kind == "A":
                err = _proto(lib, "ref_affine_picture", ctypes.c_int, ctypes.POINTER(abi.InterFrame), ctypes.c_int, ctypes.c_void_p, ctypes.c_int)(
                    pic.bd, ctypes.byref(h.f), pic.ctb_log2, h.aff.ctypes.data, len(h.aff))
            else:
                err = _proto(lib, "ref_gpm_picture", ctypes.c_int, ctypes.POINTER(abi.InterFrame), ctypes.c_int, ctypes.c_void_p, ctypes.c_int)(
                    pic.bd, ctypes.byref(h.f), pic.ctb_log2, h.gpm.ctypes.data, len(h.gpm))
            assert err == 0, f"{pic.name}: the reference shim refused the picture's {kind} units"
        elif kind == "R":
            _proto(lib, "orc_inter_frame_pass", ctypes.c_int, ctypes.POINTER(abi.InterFrame))(pic.bd, ctypes.byref(h.f))
        elif kind == "A":
            out.aff_jl, out.aff_jc = pic.expect_affine(h.plane, h.ref, lambda u: h.aff.ctypes.data + u * agc.AFFINE_CU_DT.itemsize, h.lut.ctypes.data)
            agc.call(lib.orc_affine_block, pic.bd, out.aff_jl)
            agc.call(lib.orc_bipred_block, pic.bd, out.aff_jc)
        else:
            out.gpm_jobs = pic.expect_gpm(h.plane, h.ref, h.lut.ctypes.data, GPM_MASKS.ctypes.data, GPM_TABLES)
            agc.call(lib.orc_gpm_block, pic.bd, out.gpm_jobs)
    h.untouched(side)
    out.keep = h
    return out


def run_ciip(lib, side, cp):
    """The inter half of the picture's CIIP units on the host -> scratch, planes, weights ([unit][3]).  "orc": ciip_frame_cases' restatement
    (expect_jobs through orc_bipred_block, intra_weight); "ref": ref_ciip_picture."""
    p = cp.p
    if side == "orc":
        _jobs, scratch, planes = cc.oracle_run(lib, p, cp.bd, cp.dims, cp.refs, cp.lut, cp.sentinel)
        return SimpleNamespace(scratch=scratch, planes=planes[:cp.n_comp], weights=ciip_weights(cp, cc.unit_weights(p)))
    dt = px(cp.bd)
    scratch = np.full(p.scratch_len, cp.sentinel, dt)
    planes = [np.full((ph, pw), cp.sentinel, dt) for (pw, ph) in cp.dims]
    weights = np.zeros((len(p.cus), 3), np.int32)
    refs = [[[a.copy() for a in r] for r in l] for l in cp.refs]
    mvf, cus, lut, slices = p.mvf.copy(), p.cus.copy(), cp.lut.copy(), type(p.slices).from_buffer_copy(p.slices)
    reft = cc.ref_table([[[a.ctypes.data for a in r] for r in l] for l in refs], [d[0] * p.isz for d in cp.dims])
    f = p.pic([a.ctypes.data for a in planes], [a.strides[0] for a in planes], mvf.ctypes.data, ctypes.addressof(reft), ctypes.addressof(slices), lut.ctypes.data)
    tabs = [np.ascontiguousarray(a) for a in (p.slice_idx, p.col_bd, p.row_bd)]
    fn = _proto(lib, "ref_ciip_picture", ctypes.c_int, ctypes.POINTER(abi.InterFrame), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p)
    err = fn(cp.bd, ctypes.byref(f), p.ctb_log2, cus.ctypes.data, len(cus), *(t.ctypes.data for t in tabs), scratch.ctypes.data, len(scratch), weights.ctypes.data)
    assert err == 0, f"{cp.name}: ref_ciip_picture refused the picture"
    assert np.array_equal(mvf, p.mvf) and np.array_equal(cus, p.cus) and bytes(slices) == bytes(p.slices), f"{cp.name}: ref wrote to an input table"
    return SimpleNamespace(scratch=scratch, planes=planes[:cp.n_comp], weights=weights)


# ---------------------------------------------------------------------------------------------------------------- digests

def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def mvf_bytes(a):
    """MvField entries with the pad bytes zeroed: what a digest sees of a motion field."""
    a = a.copy()
    a["pad_"] = 0
    return a.view(np.uint8).reshape(a.shape + (ifc.MVF_DT.itemsize,))


def inputs_digest(pic):
    conf = json.dumps([pic.bd, pic.idc, pic.ctb_log2, pic.width, pic.height, pic.kinds, pic.ctu_slice, pic.sentinel])
    return sha(np.frombuffer(conf.encode(), np.uint8), mvf_bytes(pic.mvf), pic.pus.view(np.uint8), pic.aff.view(np.uint8), pic.gpm.view(np.uint8),
               np.frombuffer(bytes(pic.slices), np.uint8), pic.lut, *[pic.refs[l][r][c] for l in range(2) for r in range(2) for c in range(pic.n_comp)])


def ciip_inputs_digest(cp):
    p = cp.p
    conf = json.dumps([cp.bd, p.idc, p.ctb_log2, p.width, p.height, p.scratch_len, cp.sentinel])
    return sha(np.frombuffer(conf.encode(), np.uint8), mvf_bytes(p.mvf), p.cus.view(np.uint8), p.cmds.view(np.uint8), p.slice_idx, p.col_bd, p.row_bd,
               np.frombuffer(bytes(p.slices), np.uint8), cp.lut, *[cp.refs[l][r][c] for l in range(2) for r in range(2) for c in range(cp.n_comp)])


def plane_digests(planes):
    return {f"p{c}": sha(p) for c, p in enumerate(planes)}


def picture_names():
    return REGULAR + AFFINE + GPM + CIIP + [MIXED]


def picture_digests(name, run, run_i):
    """The record of tests/golden/ref_inter.json for one listed picture, from run(pic) / run_i(cp): one digest over the inputs, one per output
    plane; regular pictures (and M0) add tab_dmvr_mvf, CIIP pictures the scratch, the intra weights and the patched .joint bytes."""
    if name in CIIP:
        cp = ciip_picture(name)
        out = run_i(cp)
        rec = {"inputs": ciip_inputs_digest(cp), **plane_digests(out.planes)}
        rec.update(scratch=sha(out.scratch), weights=sha(out.weights), joint=sha(ciip_joint(cp, out.weights)))
        return rec
    pic = picture(name)
    out = run(pic)
    rec = {"inputs": inputs_digest(pic), **plane_digests(out.planes)}
    if "R" in pic.kinds:
        rec["dmvr"] = sha(mvf_bytes(out.dmvr))
    return rec


def host_digests(lib, side, name):
    return picture_digests(name, lambda pic: run_picture(lib, side, pic), lambda cp: run_ciip(lib, side, cp))


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


# ---------------------------------------------------------------------------------------------------------------- reading a difference

def plane_differences(pic, want, got, label="reference"):
    """One line per differing component: the first differing sample and the unit that covers it."""
    lines = []
    for c, (x, y) in enumerate(zip(want, got)):
        bad = np.argwhere(x != y)
        if len(bad):
            b = tuple(int(v) for v in bad[0])
            u = pic.unit_at(c, *b) if hasattr(pic, "unit_at") else None
            where = f"in the {u[0]} unit at ({u[1]}, {u[2]}) of {u[3]}x{u[4]}" if u else "outside every unit"
            lines.append(f"{pic.name}: component {c}: {len(bad)} samples differ, first at (row, col) {list(b)} {where}: {label} {x[b]}, other side {y[b]}")
    return lines


def dmvr_differences(pic, want, got, label="reference"):
    bad = np.argwhere((mvf_bytes(want) != mvf_bytes(got)).any(-1))
    if not len(bad):
        return []
    b = tuple(int(v) for v in bad[0])
    u = pic.unit_at(0, 4 * b[0], 4 * b[1])
    return [f"{pic.name}: tab_dmvr_mvf: {len(bad)} entries differ, first at unit (row, col) {list(b)} in the unit {u}: {label} {want[b]}, other side {got[b]}"]


def ciip_differences(cp, want, got, label="reference"):
    p, lines = cp.p, []
    bad = np.nonzero(want.scratch != got.scratch)[0]
    if len(bad):
        o = int(bad[0])
        u = [i for i, cu in enumerate(p.cus) if int(cu["scratch_off"]) <= o < int(cu["scratch_off"]) + cc.region_len(int(cu["cb_width"]), int(cu["cb_height"]), p.hs, p.vs, p.chroma)]
        cu = p.cus[u[0]] if u else None
        lines.append(f"{cp.name}: scratch: {len(bad)} pixels differ, first at {o} " + (f"in unit {u[0]} at ({cu['x0']}, {cu['y0']}) of {cu['cb_width']}x{cu['cb_height']}, "
                     f"{o - int(cu['scratch_off'])} pixels into its region" if u else "outside every region") + f": {label} {want.scratch[o]}, other side {got.scratch[o]}")
    for c, (x, y) in enumerate(zip(want.planes, got.planes)):
        bad = np.argwhere(x != y)
        if len(bad):
            b = tuple(int(v) for v in bad[0])
            lx, ly = b[1] << (p.hs if c else 0), b[0] << (p.vs if c else 0)
            u = [i for i, cu in enumerate(p.cus) if cu["x0"] <= lx < cu["x0"] + cu["cb_width"] and cu["y0"] <= ly < cu["y0"] + cu["cb_height"]]
            lines.append(f"{cp.name}: component {c}: {len(bad)} samples differ, first at (row, col) {list(b)} in unit {u}: {label} {x[b]}, other side {y[b]}")
    bad = np.argwhere(want.weights != got.weights)
    if len(bad):
        u, c = (int(v) for v in bad[0])
        cu = p.cus[u]
        lines.append(f"{cp.name}: intra weight of unit {u} at ({cu['x0']}, {cu['y0']}) of {cu['cb_width']}x{cu['cb_height']}, component {c}: {label} "
                     f"{want.weights[u, c]}, other side {got.weights[u, c]}")
    return lines

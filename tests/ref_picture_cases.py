"""Whole pictures for the join of inter prediction, reconstruction and inverse LMCS, pinned against the reference's own three calls per CTU
(oracle/ref_shim_picture.c: ref_decode_picture = ff_vvc_predict_inter, ff_vvc_reconstruct — which calls ff_vvc_predict_ciip itself — and
ff_vvc_lmcs_filter on ONE set of real objects; intra.intra_pred and inter.put_ciip are the reference's own).

ONE unit-level description per picture, and both sides derived from it.  The description is a recorder_units_cases drawing (dress() on a
ref_recon_cases drawing: coding units with transform units, levels, CIIP flags and PLAIN / sub-block / AFFINE / GPM prediction units) plus
  * two reference pictures per list and the forward luma map (recorder_chain_cases.content = ciip_frame_cases.pictures: smooth_picture /
    shifted, as ref_inter_cases has them), an inverse map of random entries (any table does), both kept as data;
  * one vvc355_inter_slice per slice: its LMCS flag is the drawing's, one slice of a three-slice picture has explicit weights;
  * the MvField table of recorder_units_cases.paint_mvf with the affine PROF fields of mvf_unit_cases (held to mvf_unit_ref.json).
The destination planes start filled with a sentinel: every sample is written by some unit (covers() asserts that the units tile the picture).

  reference side   run_reference(): ref_recon_cases.mirror() (the arrays of ref_recon_picture, ciip_flag honoured), the host twin of
                   vvc355_inter_frame over the same planes, the expected vvc355_inter_pu / _affine_cu / _gpm_cu / _ciip_cu lists.
  oracle side      run_oracle(): recorder_chain_cases.inter_oracle (orc_inter_frame_pass, expect_affine / expect_gpm through orc_affine_block /
                   orc_gpm_block), ciip_oracle (the CIIP builder's restatement with orc_bipred_block, ref_recon_cases.oracle_side), a LUT lookup
                   under picture_cases.lmcs_mask.  Fed the inputs derived by INTEGRATION.md section 3 (recorder_units_cases.derive / expect_units).

Domain: ref_recon_cases' and ref_inter_cases' limits carry over and are asserted by in_domain(): no intra chroma block under 4 wide or 16
samples, the two dequant bounds (asserted where the levels are drawn), ref_idx 0 / 1 (the explicit weight tables hold 15 entries), one
slice per CTU, no CIIP unit in the regular list, sizes that are multiples of 8, no picture above 264x136.

Sensitivity (MISREADINGS, each applied to the oracle side or to the derivation of its inputs alone; SENSITIVITY names the listed pictures
that then differ from the reference; tests/test_ref_picture_cpu.py recomputes the table where the library is built):
  ciip_forward_map_after_blend        the forward map applied to a CIIP unit's luma after the blend instead of before: the inter half goes
                                      into the blend unmapped, and the map is applied to the blended luma of the units no residual follows
                                      (uncoded units under LMCS, counted as a premise; there the model is exact for the unit's own samples.
                                      Where a residual follows the blend the walk has no place for the map, and the luma stays unmapped)
  ciip_residual_before_blend          a CIIP unit's RESID commands moved between its PRED and its CIIP command
  ciip_unit_in_the_regular_list       a CIIP unit predicted onto the picture by the regular pass as well: caught by NO picture, and none can —
                                      every component the regular pass writes of such a unit is written again before anything reads it: blended
                                      components by the unit's own PRED command, unblended chroma by the CIIP stage's jobs with the same motion,
                                      and no scale of the table is read from a CTU with a CIIP unit (needs_walk counts it among the intra ones).
  scale_table_from_unmapped_luma      the forward map left off the luma that a 64x64 unit's chroma scale reads through the table
                                      (the table of a second run of the chain whose inter stages do not map)
  inverse_lmcs_on_every_ctb           inverse LMCS applied to the CTBs of a slice without lmcs_used as well
  ciip_chroma_2_wide_blended          CIIP chroma 2 wide blended like wider chroma (the reference's do_ciip needs w_c > 2, vvc_inter.c:590): those
                                      units' chroma jobs go to a scratch, PRED + CIIP commands for Cb and Cr follow the luma CIIP command
The issue's "8 wide at 4:2:2 (chroma not blended)" is, by that line of the reference, 4 wide: at 4:2:2 an 8-wide unit has chroma 4 wide,
which IS blended.  Both are counted: 4-wide units with coded chroma at 4:2:0 and at 4:2:2 (not blended), 8-wide at 4:2:2 (blended)."""
import ctypes
import json
import os
from collections import Counter
from types import SimpleNamespace

import numpy as np

import ciip_frame_cases as cf
import mvf_unit_cases as mu
import picture_cases as pcs
import recorder_chain_cases as ch
import recorder_units_cases as uc
import ref_inter_cases as ri
import ref_recon_cases as rc
from ffvvc_amd import abi

GOLDEN_PATH = os.path.join(rc.ROOT, "tests", "golden", "ref_picture.json")
SEED = 0x91C70000
SWEEP = 48

# name -> (what ref_recon_cases.draw draws, share of eligible inter units that become CIIP units, index of the slice with explicit weights or None)
_LISTED = {
    # 10 bit 4:2:0, CTU 64, three slices with LMCS on / off / on, the middle one with explicit weights; partial CTUs right and below
    "W0": (dict(bd=10, idc=1, ctb_log2=6, size=(200, 136), intra=0.3, slices=[(1, 1), (0, 0), (1, 1)], lmcs=True, min_cu=4), 0.4, 1),
    # 8 bit 4:4:4, CTU 32, tiles and wavefront
    "W1": (dict(bd=8, idc=3, ctb_log2=5, size=(136, 104), intra=0.3, tiles=True, wpp=1, slices=[(0, 1), (1, 1)], lmcs=True, explicit_mts=True), 0.4, None),
    # 12 bit 4:2:2 at range 18, CTU 128 with inter units of 128 and whole inter CTUs
    "W2": (dict(bd=12, idc=2, ctb_log2=7, size=(264, 136), intra=0.3, rbits=18, slices=[(1, 1)], lmcs=True, big_inter=True, inter_ctu=0.3, joint_sign=1,
                min_cu=4), 0.4, None),
    # 4:0:0, LMCS off
    "W3": (dict(bd=10, idc=0, ctb_log2=6, size=(136, 72), intra=0.4, min_cu=4, slices=[(0, 0), (1, 0)], explicit_mts=True), 0.5, None),
    # 4:2:0 with tiles, three slices, mostly inter CTUs around a few intra ones: LIGHT CTUs beside CIIP units
    "W4": (dict(bd=10, idc=1, ctb_log2=6, size=(264, 136), intra=0.35, inter_ctu=0.5, min_cu=4, tiles=True, slices=[(1, 1), (0, 1), (1, 0)], lmcs=True,
                explicit_mts=True, joint_sign=1), 0.35, 2),
    # 12 bit 4:4:4 at CTU 32 with units down to 4x4
    "W5": (dict(bd=12, idc=3, ctb_log2=5, size=(72, 72), intra=0.4, min_cu=4, slices=[(0, 1)], lmcs=True), 0.5, None),
    # 8 bit 4:2:0, CTU 128, wavefront, LMCS mixed per slice
    "W6": (dict(bd=8, idc=1, ctb_log2=7, size=(200, 136), intra=0.3, slices=[(0, 0), (1, 1)], lmcs=True, wpp=1, min_cu=4), 0.4, None),
    # 10 bit 4:2:0 at CTU 32, no joint Cb-Cr, most CTUs wholly inter and few CIIP units: most chroma scales go through the table
    "W7": (dict(bd=10, idc=1, ctb_log2=5, size=(264, 136), intra=0.15, inter_ctu=0.8, slices=[(1, 1)], lmcs=True, tools=dict(joint=0.0)), 0.1, None),
    # 8 bit 4:2:2, CTU 32, no LMCS at all
    "W8": (dict(bd=8, idc=2, ctb_log2=5, size=(136, 104), intra=0.4, slices=[(0, 0)], explicit_mts=True, min_cu=4), 0.5, None),
    # 10 bit 4:2:2, CTU 64, tiles, LMCS; more MIP and CCLM units than elsewhere, beside inter units of every kind
    "W9": (dict(bd=10, idc=2, ctb_log2=6, size=(200, 136), intra=0.35, tiles=True, slices=[(1, 1), (1, 0)], lmcs=True, min_cu=4, joint_sign=1,
                tools=dict(mip=0.35, cclm=0.5)), 0.4, None),
}
RASTER_TOO = ("W0", "W5")                      # the pictures the GPU test also runs with the CTUs in raster ticket order

MISREADINGS = ("ciip_forward_map_after_blend", "ciip_residual_before_blend", "ciip_unit_in_the_regular_list", "scale_table_from_unmapped_luma",
               "ciip_chroma_2_wide_blended", "inverse_lmcs_on_every_ctb")
SENSITIVITY = {
    "ciip_chroma_2_wide_blended": ["W0", "W2", "W4", "W6", "W8", "W9"],
    "ciip_forward_map_after_blend": ["W0", "W1", "W2", "W4", "W5", "W6", "W7", "W9"],
    "ciip_residual_before_blend": ["W0", "W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9"],
    "ciip_unit_in_the_regular_list": [],
    "scale_table_from_unmapped_luma": ["W7"],
    "inverse_lmcs_on_every_ctb": ["W0", "W3", "W4", "W6", "W8", "W9"],
}


# ---------------------------------------------------------------------------------------------------------------- drawing

def weighted_slices(rng, n, which):
    """One vvc355_inter_slice per slice, default weights but slice `which`: B-typed with explicit weights (as ref_inter_cases.make_slices)."""
    slices = (abi.InterSlice * n)()
    if which is not None:
        s = slices[which]
        s.weighted_bipred = 1
        s.log2_denom[0], s.log2_denom[1] = 6, 5
        for l in range(2):
            for c in range(3):
                for r in range(16):
                    s.weight[l][c][r] = int(rng.integers(-32, 96))
                    s.offset[l][c][r] = int(rng.integers(-20, 21))
    return slices


def finish(pic, rng, which):
    """What the description adds to a dressed drawing: sentinel-filled planes, the slice table, the inverse map."""
    pic.sentinel = (1 << pic.bd) // 3
    pic.planes = [np.full(p.shape, pic.sentinel, p.dtype) for p in pic.planes]
    pic.inter_slices = weighted_slices(rng, len(pic.slices), which)
    pic.inv_lut = rng.integers(0, 1 << pic.bd, size=1 << pic.bd, dtype=np.int64).astype(pic.planes[0].dtype)
    pic._flat = None
    return pic


_pictures, _inputs = {}, {}


def picture_names():
    return list(_LISTED)


def picture(name):
    """A listed picture; made once, nobody writes to it."""
    if name not in _pictures:
        kw, frac, which = _LISTED[name]
        k = list(_LISTED).index(name)
        pic = uc.dress(rc.draw(name, SEED + k, **kw), 5000 + k, frac)
        _pictures[name] = finish(pic, np.random.default_rng([SEED, 1, k]), which)
    return _pictures[name]


def sweep_picture(k):
    """Freshly drawn picture k of the sweep: ref_recon_cases.sweep_picture's free draw (size, format, depth, CTU, flags, unit mix) dressed
    with CIIP units and motion; a picture of three slices gets explicit weights in one of them."""
    rng = np.random.default_rng([SEED, 2, k])
    pic = uc.dress(rc.sweep_picture(k, salt=11), 7000 + k, float(rng.choice([0.0, 0.3, 0.6])))
    return finish(pic, rng, int(rng.integers(0, 3)) if len(pic.slices) == 3 else None)


# ---------------------------------------------------------------------------------------------------------------- the domain

def covers(pic):
    """Every luma sample lies in exactly one luma-tree unit, every chroma sample (where there is chroma) in exactly one chroma-tree unit."""
    for tree in (0, 1):
        n = np.zeros((pic.height, pic.width), np.int32)
        for ctu in pic.ctus:
            for cu in ctu:
                if cu["tree_type"] != (1, 2)[1 - tree] and (tree == 0 or pic.idc):
                    n[cu["y0"]:cu["y0"] + cu["h"], cu["x0"]:cu["x0"] + cu["w"]] += 1
        if (tree == 0 or pic.idc) and not np.all(n == 1):
            return False
    return True


def in_domain(pic):
    """None, or the first limit of the module docstring the description breaks (the generator alone has to stay inside)."""
    ctb = 1 << pic.ctb_log2
    if pic.width > 264 or pic.height > 136 or pic.width % 8 or pic.height % 8:
        return "size"
    if not covers(pic):
        return "the units do not tile the picture"
    if len(pic.inter_slices) != len(pic.slices) or len(pic.slices) > 8:
        return "slice table"
    for s in pic.inter_slices:
        if s.weighted_pred and s.weighted_bipred:
            return "a slice with both weighted-prediction switches"
    for rs, ctu in enumerate(pic.ctus):
        for cu in ctu:
            x, y, w, h = cu["x0"], cu["y0"], cu["w"], cu["h"]
            if (x // ctb, y // ctb) != (rs % pic.ncx, rs // pic.ncx) or (x + w - 1) // ctb != x // ctb or (y + h - 1) // ctb != y // ctb:
                return "a unit outside its CTU (one slice per CTU)"
            if cu["pred_mode"] == 1 and cu["tree_type"] != 1 and pic.idc and ((w >> pic.hs) < 4 or (w >> pic.hs) * (h >> pic.vs) < 16):
                return "an intra chroma block under 4 wide or 16 samples"
            if cu["ciip_flag"] and not uc.ciip_eligible(cu):
                return "a CIIP unit outside 4..64 a side and 64 samples"
            pu = cu.get("pu")
            if (cu["pred_mode"] != 1 and cu["tree_type"] != 2) != (pu is not None):
                return "a unit with inter luma and no prediction unit"
            if pu is None:
                continue
            if cu["ciip_flag"] and (pu["kind"] != mu.PLAIN or pu["nsx"] * pu["nsy"] != 1 or pu["dmvr"] or pu["bdof"]):
                return "a CIIP unit that the regular list would hold"
            if w & (w - 1) or h & (h - 1) or w < 4 or h < 4 or (x | y) & 3:
                return "a unit the inter callers cannot hold"
            refs = pu["ref_idx"] if pu["kind"] == mu.AFFINE else [int(v) for m in pu["motion"].view(uc.MVF) for v in m["ref_idx"]]
            if max(refs) > 1:
                return "ref_idx above 1"
    return None


# ---------------------------------------------------------------------------------------------------------------- both sides' inputs

def inputs(pic):
    """Everything both sides are fed, derived once per picture: d (recorder_units_cases.derive), e (expect_units, the affine records with
    their PROF fields), mvf, the CIIP picture p, dims / refs / lut."""
    key = id(pic)
    if key not in _inputs:
        d = uc.derive(pic)
        e = uc.expect_units(pic, d)
        g = mu.Geo(pic.width, pic.height, pic.ctb_log2)
        e.affine = e.affine.copy()
        mvf = uc.paint_mvf(pic, np.zeros((g.th, g.tw), mu.MVF_DT), e.affine)
        p = ch.ciip_inputs(pic, e, d.cmds)
        dims, refs, lut = ch.content(pic, p)
        _inputs[key] = SimpleNamespace(pic=pic, d=d, e=e, mvf=mvf, p=p, dims=dims, refs=refs, lut=lut, n=3 if pic.idc else 1)
    return _inputs[key]


def mvf_bytes(a):
    return ri.mvf_bytes(np.ascontiguousarray(a).view(ri.ifc.MVF_DT).reshape(a.shape))


# ---------------------------------------------------------------------------------------------------------------- the oracle side

def _per_unit(cmds):
    """The command array cut into runs of one coding unit each (a unit's commands are contiguous and carry its origin)."""
    key = cmds["cu_x0"].astype(np.int64) << 20 | cmds["cu_y0"]
    cuts = np.nonzero(np.diff(key))[0] + 1
    return np.split(cmds, cuts)


def _resid_first(unit):
    """One unit's commands with every RESID command of a component moved between that component's PRED and CIIP command; a unit without a
    CIIP command comes back as it is."""
    out = list(range(len(unit)))
    for c in range(3):
        at = [k for k in range(len(unit)) if unit["kind"][k] == abi.RECON_CIIP and unit["c_idx"][k] == c]
        res = [k for k in range(len(unit)) if unit["kind"][k] == abi.RECON_RESID and unit["c_idx"][k] == c]
        if at and res:
            out = [k for k in out if k not in res]
            where = out.index(at[0])
            out[where:where] = res
    return unit[out]


class _Blend2:
    """The misreading 'CIIP chroma 2 wide blended' on the oracle side alone: the chroma jobs of the CIIP units whose chroma is 2 wide go
    to a scratch of their own instead of the planes, and each such unit gets PRED + CIIP commands for Cb and Cr after its luma CIIP command,
    with the unit's intra weight, as the units with wider chroma have them.  The CTU table's ranges follow."""

    def __init__(self, pic):
        self.pic, self.off = pic, {}

    def _narrow(self, p):
        return [cu for cu in p.cus if p.chroma and (int(cu["cb_width"]) >> p.hs) <= 2]

    def jobs(self, p, jobs):
        n = sum(2 * (int(cu["cb_width"]) >> p.hs) * (int(cu["cb_height"]) >> p.vs) for cu in self._narrow(p))
        self.scratch = np.zeros(max(1, n), self.pic.planes[0].dtype)
        at = 0
        for cu in self._narrow(p):
            w, h = int(cu["cb_width"]), int(cu["cb_height"])
            wc, hc = w >> p.hs, h >> p.vs
            for k, (c, tx, ty, tw, th) in enumerate(cf.tiles_of(w, h, p.hs, p.vs, p.chroma)):
                if c:
                    j = jobs[int(cu["first_job"]) + k]
                    j["dst"], j["dst_stride"] = self.scratch.ctypes.data + (at + (c - 1) * wc * hc + ty * wc + tx) * p.isz, wc * p.isz
            self.off[(int(cu["x0"]), int(cu["y0"]))] = at
            at += 2 * wc * hc

    def cmds(self, p, d2):
        units, ctus, added = [], d2.ctus.copy(), []             # added: the old indices ahead of which four commands go in
        old = 0
        for unit in _per_unit(d2.cmds):
            n_old = len(unit)
            org = (int(unit["cu_x0"][0]), int(unit["cu_y0"][0]))
            luma = [k for k in range(len(unit)) if unit["kind"][k] == abi.RECON_CIIP and unit["c_idx"][k] == 0]
            if org in self.off and luma:
                x0, y0, w, h = org[0], org[1], int(unit["cb_width"][0]), int(unit["cb_height"][0])
                wc, hc = w >> p.hs, h >> p.vs
                new = []
                for c in (1, 2):
                    new.append(uc._cmd(abi.RECON_PRED, c, x0, y0, w, h, x0, y0, w, h, mode=0))
                    new.append(uc._cmd(abi.RECON_CIIP, c, x0, y0, w, h, x0, y0, w, h, resid=self.scratch.ctypes.data + (self.off[org] + (c - 1) * wc * hc) * p.isz,
                                       joint=cf.intra_weight(p, x0, y0, w, h)))
                unit = np.concatenate([unit[:luma[0] + 1], np.array(new, rc.CMD), unit[luma[0] + 1:]])
                added.append(old + luma[0] + 1)
            units.append(unit)
            old += n_old
        for rs in np.nonzero(ctus["n_cmd"])[0]:
            first, n = int(ctus[rs]["first_cmd"]), int(ctus[rs]["n_cmd"])
            ctus[rs]["first_cmd"] = first + 4 * sum(a <= first for a in added)
            ctus[rs]["n_cmd"] = n + 4 * sum(first < a <= first + n for a in added)
        assert len(added) == len(self.off), "a CIIP unit with 2-wide chroma without its luma CIIP command"
        d2.cmds, d2.ctus = np.concatenate(units), ctus


def run_oracle(orc, pic, misread=None):
    """The existing chain on the derived inputs -> recon / final planes, tab_dmvr_mvf, the scale table (or None) and d."""
    assert misread is None or misread in MISREADINGS
    i = inputs(pic)
    d, e = i.d, i.e
    if misread == "ciip_unit_in_the_regular_list":
        e = SimpleNamespace(**vars(e))
        extra = [(int(c["x0"]), int(c["y0"]), int(c["cb_width"]), int(c["cb_height"]), 1, 1, 0, 0, 0, int(c["hpel_if_idx"]), int(c["slice"]), 0, 0) for c in e.ciip]
        e.inter = np.concatenate([e.inter, np.array(extra, uc.INTER_PU)]) if extra else e.inter
        tiles = [uc.tiles16(int(c["cb_width"])) * uc.tiles16(int(c["cb_height"])) for c in i.e.ciip]
        e.inter["first_job"][len(i.e.inter):] = i.e.totals["n_inter_jobs"] + np.concatenate(([0], np.cumsum(tiles)[:-1])) if extra else []
        e.totals = dict(e.totals, n_inter_jobs=e.totals["n_inter_jobs"] + int(sum(tiles)))
    scale_table = None
    if misread == "scale_table_from_unmapped_luma" and pic.chroma_scale_flag:
        # the whole chain once more with the forward map off in the three inter stages: its scale table is the one of unmapped luma
        plain = type(i.p.slices).from_buffer_copy(i.p.slices)
        for s in plain:
            s.lmcs_used = 0
        unmapped = ch.inter_oracle(orc, pic, e, i.mvf.copy(), e.affine.copy(), i.refs, i.lut, i.dims, plain, [p.copy() for p in pic.planes])
        scale_table = ch.ciip_oracle(orc, pic, d, i.e, i.refs, i.lut, i.dims, start=unmapped, whole=True)[1]
    dmvr = i.mvf.copy()
    start = ch.inter_oracle(orc, pic, e, i.mvf.copy(), e.affine.copy(), i.refs, i.lut, i.dims, i.p.slices, [p.copy() for p in pic.planes], dmvr=dmvr)

    jobs_hook = cmds_hook = None
    after_blend = misread == "ciip_forward_map_after_blend"
    if after_blend:
        def jobs_hook(p, jobs):
            jobs["lmcs_lut"] = 0
    if misread == "ciip_residual_before_blend":
        def cmds_hook(p, d2):
            d2.cmds = np.concatenate([_resid_first(c) for c in _per_unit(d2.cmds)])
    if misread == "ciip_chroma_2_wide_blended":
        keep = _Blend2(pic)
        jobs_hook, cmds_hook = keep.jobs, keep.cmds
    recon, table = ch.ciip_oracle(orc, pic, d, i.e, i.refs, i.lut, i.dims, start=start, whole=True, jobs_hook=jobs_hook, cmds_hook=cmds_hook,
                                  scale_table=scale_table)
    if after_blend:
        # the map the blend's input did not get, on the blended luma: exact for the unit's own samples where no residual follows the blend
        for rs, ctu in enumerate(pic.ctus):
            for cu in ctu:
                if cu["ciip_flag"] and not cu["coded_flag"] and pic.slices[int(pic.slice_idx[rs])][1]:
                    s_ = np.s_[cu["y0"]:cu["y0"] + cu["h"], cu["x0"]:cu["x0"] + cu["w"]]
                    recon[0][s_] = i.lut[recon[0][s_]]
    used = np.array([1 if misread == "inverse_lmcs_on_every_ctb" else sl[1] for sl in pic.slices], np.uint8)
    mask = pcs.lmcs_mask(pic.width, pic.height, pic.ctb_log2, pic.slice_idx, used)
    final = [np.where(mask, pic.inv_lut[recon[0]], recon[0]).astype(recon[0].dtype)] + [p.copy() for p in recon[1:]]
    return SimpleNamespace(recon=recon[:i.n], final=final[:i.n], dmvr=dmvr, table=table, d=d, mask=mask)


# ---------------------------------------------------------------------------------------------------------------- the reference side

def bind_reference(lib):
    rc.bind_reference(lib)
    lib.ref_decode_picture.argtypes = [ctypes.POINTER(rc.MirReconPic), ctypes.POINTER(abi.InterFrame), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p * 3)]
    lib.ref_decode_picture.restype = ctypes.c_int


def run_reference(lib, pic, change=None):
    """ref_decode_picture over the picture -> ret, recon / final planes, tab_dmvr_mvf, the scales the reference cached and the units it cached
    two values for.  change(m, f, lists): edits the arguments before the call (the refusal tests)."""
    bind_reference(lib)
    i = inputs(pic)
    e = i.e
    planes = [p.copy() for p in pic.planes]
    recon = [np.zeros_like(p) for p in planes]
    log = np.zeros((4 * len(rc.shim_arrays(pic)[3]) + 4, 3), np.int32)
    m, _keep = rc.mirror(pic, planes, log)
    mvf, dmvr = i.mvf.copy(), i.mvf.copy()
    refs = [[[a.copy() for a in r] for r in l] for l in i.refs]
    reft = cf.ref_table([[[a.ctypes.data for a in r] for r in l] for l in refs], [dm[0] * pic.isz for dm in i.dims])
    lut, inv, slices = i.lut.copy(), pic.inv_lut.copy(), type(i.p.slices).from_buffer_copy(i.p.slices)
    lists = SimpleNamespace(inter=np.ascontiguousarray(e.inter).copy(), affine=e.affine.copy(), gpm=np.ascontiguousarray(e.gpm).copy(),
                            ciip=np.ascontiguousarray(e.ciip).copy())
    f = i.p.pic([p.ctypes.data for p in planes], [p.strides[0] for p in planes], mvf.ctypes.data, ctypes.addressof(reft), ctypes.addressof(slices), lut.ctypes.data)
    f.dmvr_mvf = dmvr.ctypes.data
    if change is not None:
        change(m, f, lists)
    f.pus, f.n_pus = lists.inter.ctypes.data, len(lists.inter)
    out = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in recon])
    levels = rc.shim_arrays(pic)[4]
    before = levels.copy()
    ret = lib.ref_decode_picture(ctypes.byref(m), ctypes.byref(f), lists.affine.ctypes.data, len(lists.affine), lists.gpm.ctypes.data, len(lists.gpm),
                                 lists.ciip.ctypes.data, len(lists.ciip), inv.ctypes.data, ctypes.byref(out))
    assert np.array_equal(levels, before) and m.n_scale_log <= len(log)
    assert np.array_equal(mvf, i.mvf) and np.array_equal(lut, i.lut) and bytes(slices) == bytes(i.p.slices), f"{pic.name}: the reference wrote to an input"
    scales, twice = rc.scales_of(log, m.n_scale_log)
    return SimpleNamespace(ret=ret, recon=recon[:i.n], final=planes[:i.n], dmvr=dmvr, scales=scales, twice=twice)


def reference_table(pic, d, scales):
    """The scale table reduced to the routed units, from what the reference cached (None without chroma residual scaling)."""
    if d.tpic.model is None:
        return None
    table = np.zeros((d.tpic.uy, d.tpic.ux), np.int16)
    for (ux, uy) in d.routed:
        table[uy, ux] = scales[(ux * pic.size_y, uy * pic.size_y)]
    return table


# ---------------------------------------------------------------------------------------------------------------- digests

def inputs_digest(pic):
    i = inputs(pic)
    e = i.e
    conf = json.dumps([pic.sentinel, {k: int(v) for k, v in e.totals.items()}])
    return rc.sha(np.frombuffer(rc.inputs_digest(pic).encode(), np.uint8), np.frombuffer(conf.encode(), np.uint8), mvf_bytes(i.mvf), e.inter.view(np.uint8),
                  e.affine.view(np.uint8), e.gpm.view(np.uint8), e.ciip.view(np.uint8), np.frombuffer(bytes(i.p.slices), np.uint8), i.lut, pic.inv_lut,
                  *[i.refs[l][r][c] for l in range(2) for r in range(2) for c in range(i.n)])


def digests(pic, d, recon, final, dmvr, table):
    out = {"inputs": inputs_digest(pic)}
    out.update({f"r{c}": rc.sha(p) for c, p in enumerate(recon)})
    out.update({f"p{c}": rc.sha(p) for c, p in enumerate(final)})
    out["dmvr"] = rc.sha(mvf_bytes(dmvr))
    out["scale"] = rc.scale_digest(d, table)
    return out


def reference_digests(lib, name):
    pic = picture(name)
    r = run_reference(lib, pic)
    assert r.ret == 0 and not r.twice, (name, r.ret, r.twice)
    d = inputs(pic).d
    return digests(pic, d, r.recon, r.final, r.dmvr, reference_table(pic, d, r.scales))


def oracle_digests(orc, name):
    pic = picture(name)
    o = run_oracle(orc, pic)
    return digests(pic, o.d, o.recon, o.final, o.dmvr, o.table)


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


# ---------------------------------------------------------------------------------------------------------------- what the pictures reach

def _unit_at(pic, x, y):
    for cu in pic.ctus[(y >> pic.ctb_log2) * pic.ncx + (x >> pic.ctb_log2)]:
        if cu["tree_type"] != 2 and cu["x0"] <= x < cu["x0"] + cu["w"] and cu["y0"] <= y < cu["y0"] + cu["h"]:
            return cu
    return None


def _kind(cu):
    if cu["pred_mode"] == 1:
        return "intra"
    if cu["ciip_flag"]:
        return "ciip"
    pu = cu["pu"]
    if pu["kind"] == mu.AFFINE:
        return "affine"
    if pu["kind"] == mu.GPM:
        return "gpm"
    return "regular with dmvr or bdof" if (pu["dmvr"] or pu["bdof"]) else "regular"


def census(pic, ref=None):
    """{premise: count} from the description and the derived inputs; ref: a run_reference() result, for what only its outputs show."""
    i = inputs(pic)
    d, p = i.d, i.p
    n, ctb = Counter(), 1 << pic.ctb_log2
    n[f"bit depth {pic.bd}"] += 1
    n[f"format {pic.idc}"] += 1
    n[f"ctu {ctb}"] += 1
    n[f"ctu {ctb} with partial ctus right and below"] += bool(pic.width % ctb and pic.height % ctb)
    used = [sl[1] for sl in pic.slices]
    n["lmcs on"] += all(used)
    n["lmcs off"] += not any(used)
    n["lmcs mixed per slice"] += any(used) and not all(used)
    n["three slices, one with explicit weights"] += len(pic.slices) == 3 and any(s.weighted_bipred or s.weighted_pred for s in pic.inter_slices)
    n["tiles"] += len(set(pic.col_bd[:-1].tolist())) > 1
    n["wavefront"] += pic.wpp
    n.update({k: v for k, v in uc.census(pic, d).items() if "ciip" in k})
    weights = cf.unit_weights(p)
    has_ciip = [any(cu["ciip_flag"] for cu in ctu) for ctu in pic.ctus]
    k = 0
    for rs, ctu in enumerate(pic.ctus):
        rx, ry = rs % pic.ncx, rs // pic.ncx
        left, up = cf.neighbour_flags(p, rx, ry)
        sl = pic.slices[int(pic.slice_idx[rs])]
        for cu in ctu:
            if cu["tree_type"] == 2 or (cu["pred_mode"] != 1 and not cu["ciip_flag"]):
                continue
            x, y = cu["x0"], cu["y0"]
            near = [_unit_at(pic, xx, yy) for xx, yy, ok in ((x - 1, y, x % ctb), (x, y - 1, y % ctb)) if ok]         # written by a unit of the same CTU
            if cu["ciip_flag"]:
                n[f"ciip unit with intra weight {int(weights[k])}"] += 1
                k += 1
                for o in near:
                    n[f"ciip unit beside a unit of its ctu: {_kind(o)}"] += 1
                n["ciip unit with nothing available"] += not (x % ctb or left) and not (y % ctb or up)
                n["ciip unit behind a slice edge"] += bool(y % ctb == 0 and ry and pic.slice_idx[rs] != pic.slice_idx[rs - pic.ncx])
                n["ciip unit behind a tile edge"] += bool(x % ctb == 0 and rx and pic.col_bd[rx] != pic.col_bd[rx - 1])
                n["ciip unit under lmcs" if sl[1] else "ciip unit without lmcs"] += 1
                n["4-wide ciip unit at 4:2:0, chroma not blended"] += pic.idc == 1 and cu["w"] == 4
                n["4-wide ciip unit at 4:2:2, chroma not blended"] += pic.idc == 2 and cu["w"] == 4
                coded_c = bool(cu["coded_flag"]) and any(b["c_idx"] and b["has"] for tu in cu["tus"] for b in tu["tbs"])
                n["4-wide ciip unit at 4:2:0 with coded chroma, not blended"] += pic.idc == 1 and cu["w"] == 4 and coded_c
                n["4-wide ciip unit at 4:2:2 with coded chroma, not blended"] += pic.idc == 2 and cu["w"] == 4 and coded_c
                n["uncoded ciip unit under lmcs"] += bool(sl[1]) and not cu["coded_flag"]
            else:
                tools = ([("angular", not cu["mip_flag"] and 2 <= cu["mode_y"] <= 66), ("mip", bool(cu["mip_flag"]))] if cu["tree_type"] != 2 else []) + \
                        [("cclm", bool(pic.idc) and cu["tree_type"] != 1 and 81 <= cu["mode_c"] <= 83)]
                for o in near:
                    for t, on in tools:
                        if on and _kind(o) in ("regular with dmvr or bdof", "affine", "gpm"):
                            n[f"intra {t} unit beside a unit of its ctu: {_kind(o)}"] += 1
    n["64x64 unit scaled from inter-predicted luma through the table"] += len(d.routed)
    n["64x64 unit scaled from inter-predicted luma in the walk"] += d.stats["walk_scaled"]
    for rs in np.nonzero(d.kind == 1)[0]:
        rx, ry = rs % pic.ncx, rs // pic.ncx
        n["light ctu beside a ctu with a ciip unit"] += bool((rx and has_ciip[rs - 1]) or (ry and has_ciip[rs - pic.ncx]) or (rx + 1 < pic.ncx and has_ciip[rs + 1]))
    if ref is not None:
        moved = np.abs(ref.dmvr["mv"].astype(np.int64) - i.mvf["mv"]).max(axis=(2, 3))
        n["dmvr sub-block refined by a sample or more: reads beyond its unrefined window"] += int(np.sum(moved[::4, ::4] >= 16))
        n["dmvr sub-block refined"] += int(np.sum(moved[::4, ::4] > 0))
        mask = pcs.lmcs_mask(pic.width, pic.height, pic.ctb_log2, pic.slice_idx, np.array(used, np.uint8))
        changed = ref.final[0] != ref.recon[0]
        n["inverse lmcs changes some ctbs and leaves the others byte for byte"] += bool(mask.any() and not mask.all() and changed[mask].any() and not changed[~mask].any())
    return n


PREMISES = (["bit depth 8", "bit depth 10", "bit depth 12", "format 0", "format 1", "format 2", "format 3", "ctu 32 with partial ctus right and below",
             "ctu 64 with partial ctus right and below", "ctu 128 with partial ctus right and below", "lmcs on", "lmcs off", "lmcs mixed per slice",
             "three slices, one with explicit weights", "tiles", "wavefront",
             "ciip unit with intra weight 1", "ciip unit with intra weight 2", "ciip unit with intra weight 3"] +
            [f"ciip unit beside a unit of its ctu: {k}" for k in ("regular with dmvr or bdof", "affine", "gpm", "intra")] +
            ["ciip unit with nothing available", "ciip unit behind a slice edge", "ciip unit behind a tile edge", "ciip unit under lmcs", "ciip unit without lmcs",
             "ciip unit with a luma residual", "ciip unit with a joint cb-cr unit", "ciip unit with a transform-skip block", "uncoded ciip unit",
             "4-wide ciip unit at 4:2:0, chroma not blended", "4-wide ciip unit at 4:2:2, chroma not blended", "8-wide ciip unit at 4:2:2, blended chroma",
             "4-wide ciip unit at 4:2:0 with coded chroma, not blended", "4-wide ciip unit at 4:2:2 with coded chroma, not blended",
             "uncoded ciip unit under lmcs"] +
            [f"intra {t} unit beside a unit of its ctu: {k}" for t in ("angular", "mip", "cclm") for k in ("regular with dmvr or bdof", "affine", "gpm")] +
            ["64x64 unit scaled from inter-predicted luma through the table", "64x64 unit scaled from inter-predicted luma in the walk",
             "light ctu beside a ctu with a ciip unit"])
REFERENCE_PREMISES = ["dmvr sub-block refined by a sample or more: reads beyond its unrefined window",
                      "inverse lmcs changes some ctbs and leaves the others byte for byte"]

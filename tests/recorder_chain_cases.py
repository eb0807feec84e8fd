"""The chained oracle of a recorded picture and the picture on the device, for the tests that run the recorder's lists through the stage
drivers (tests/test_recorder_units_gpu.py, tests/test_ref_picture_cpu.py, tests/test_ref_picture_gpu.py).

  ciip_inputs()    the ciip_frame_cases.CiipPicture of a recorder_units_cases picture
  content()        its reference pictures and forward luma map
  RecordedCiip     the picture recorded, checked against the expectation and uploaded; the stages' frames filled from the two results
  inter_oracle()   the three kinds of inter units that predict onto the picture, through the oracle's block functions
  ciip_oracle()    the inter half of the CIIP units, then ref_recon_cases.oracle_side with the CIIP commands completed

A picture may carry `inter_slices` (an abi.InterSlice array, one per slice: explicit weights); without it every slice has default weights.
Both take the slice's LMCS flag from the picture's slices."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np

import ciip_frame_cases as cf
import inter_tb_cases as tc
import mvf_unit_cases as mu
import picture_cases as pcs
import recorder_cases as rk
import recorder_units_cases as uc
import ref_recon_cases as rc
from ffvvc_amd import abi, batch


def checked_record(dev, pic, d, rec=None, order=None):
    """The picture through the recorder; nothing that differs from the expectation, and no malformed ticket order, reaches the device."""
    o = uc.record(dev, pic, True, rec=rec, order=order)
    bad = rk.differences(dev, pic, d, o, True) + uc.unit_differences(pic, d, o)
    assert not bad, f"{pic.name}: {bad} differ from the expectation: not launched"
    assert pcs.order_check(dev, o.ctus, pic.ncx, pic.ncy, o.order) == 0 and rc.order_defect(o.ctus, pic.ncx, pic.ncy, o.order) is None, "not launched"
    return o



def ciip_inputs(pic, o_or_e, cmds):
    """The ciip_frame_cases.CiipPicture of a recorded picture: geometry, the MvField table painted from the units, one vvc355_inter_slice per
    slice (default weighting, lmcs_used = the slice's flag), the vvc355_ciip_cu list and the command array."""
    p = cf.CiipPicture(pic.width, pic.height, pic.ctb_log2, pic.idc, pic.isz)
    p.bd = pic.bd
    p.mvf = uc.paint_mvf(pic, np.zeros((pic.height // 4, pic.width // 4), mu.MVF_DT))
    p.slice_idx, p.col_bd, p.row_bd = pic.slice_idx, pic.col_bd, pic.row_bd
    p.n_slices = len(pic.slices)
    given = getattr(pic, "inter_slices", None)
    p.slices = (abi.InterSlice * p.n_slices)() if given is None else type(given).from_buffer_copy(given)
    assert len(p.slices) == p.n_slices
    for i, sl in enumerate(pic.slices):
        p.slices[i].lmcs_used = int(sl[1])
    p.cus, p.n_jobs, p.scratch_len = o_or_e.ciip, o_or_e.totals["n_ciip_jobs"], o_or_e.totals["ciip_scratch_len"]
    p.cmds = cmds
    return p


def content(pic, p):
    """(dims, refs[list][ref][component], forward map) of a picture: ciip_frame_cases.pictures, seeded by the bit depth; a picture may carry
    its own `content(p)` instead (the quiet pictures of ref_decoded_cases)."""
    own = getattr(pic, "content", None)
    return own(p) if own is not None else cf.pictures(np.random.default_rng([uc.SEED, pic.bd]), p, pic.bd)


class GuardedPlane:
    """A pitched plane on the device with `guard` rows of tc.FILL bytes above and below it; .ptr is the plane's first row."""

    def __init__(self, k, host, guard):
        h = host.shape[0]
        self.rows, self.full = (guard, guard + h), np.zeros((h + 2 * guard, host.shape[1]), host.dtype)
        self.full.view(np.uint8)[:] = tc.FILL
        self.full[guard:guard + h] = host
        self.buf = k.up(self.full)
        self.ptr = self.buf.ptr + guard * host.strides[0]

    def to_host(self, dtype, shape):
        got = self.buf.to_host(self.full.dtype, self.full.shape)
        a, b = self.rows
        assert np.array_equal(got[:a], self.full[:a]) and np.array_equal(got[b:], self.full[b:]), "the rows around a plane were written"
        assert got[a:b].shape == tuple(shape) and got.dtype == dtype
        return got[a:b]


def recorded_stages(k, dev, pic, d, o, cmds, d_arena, d_planes, strides, ticket):
    """The frames of the three TB record passes, the scale pass and the RECON walk from a recorder's snapshot `o`, its arrays uploaded as they
    are through the pcs.Keep `k`: (stages, scaled, the device scale table, the device command array, the device slice / column / row maps)."""
    res, bd = o.res, pic.bd
    d_slice, d_col, d_row = (k.up(a) for a in (pic.slice_idx, pic.col_bd, pic.row_bd))
    d_model = k.up(np.frombuffer(bytes(pic.model), np.uint8))
    d_levels = k.up(o.levels)
    n_i, n_e, n_s = res.n_intra, res.n_inter, res.n_ts

    def side(first, n):
        return k.up(o.lv[first:first + n].view(np.uint8) if n else np.zeros(16, np.uint8)).ptr

    scaled = bool(pic.chroma_scale_flag)
    d_table = k.up(np.full(d.tpic.ux * d.tpic.uy, -1, np.int16))
    st = {}
    if n_i:
        f = abi.IntraTbFrame()
        f.tus, f.coeffs, f.n_tus = k.up(o.intra).ptr, d_arena.ptr, n_i
        for c in range(6):
            f.class_first[c] = res.class_first[c]
        f.range, f.bd = pic.rbits, bd
        f.lv, f.levels = side(0, n_i), d_levels.ptr
        st["intra_tb"] = k.frame(f)
    for name, ty, recs, n, first, first_lv in (("inter_tb", abi.InterTbFrame, o.inter, n_e, res.bin_first, n_i),
                                               ("ts_tb", abi.TsTbFrame, o.ts, n_s, res.ts_first, n_i + n_e)):
        if not n:
            continue
        f = ty()
        f.tus, f.coeffs, f.n_tus = k.up(recs).ptr, d_arena.ptr, n
        for c in range(3):
            f.plane[c], f.stride[c] = d_planes[c].ptr, strides[c]
        f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = pic.width, pic.height, pic.hs, pic.vs, pic.size_y, pic.rbits, bd
        f.scale_table = d_table.ptr if scaled else 0
        dst = f.bin_first if name == "inter_tb" else f.class_first
        for ch in range(2):
            for b in range(len(first[ch])):
                dst[ch][b] = first[ch][b]
        f.lv, f.levels = side(first_lv, n), d_levels.ptr
        st[name] = k.frame(f)
    if scaled:
        st["lmcs_scale"] = k.frame(rc.scale_frame(pic, d_planes[0].ptr, strides[0], d_table.ptr, d_model.ptr, d_slice.ptr, d_col.ptr, d_row.ptr))
    d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(pic.ncx * pic.ncy))
    k.keep.append(d_state)
    d_cmds = k.up(cmds)
    st["recon"] = k.frame(rc.recon_frame(pic, None, [b.ptr for b in d_planes], strides, d_cmds.ptr, k.up(o.ctus).ptr, k.up(ticket).ptr,
                                         d_state.ptr, d_slice.ptr, d_col.ptr, d_row.ptr, d_model.ptr if scaled else 0, n_work=res.n_work))
    return st, scaled, d_table, d_cmds, (d_slice, d_col, d_row)


class RecordedCiip:
    """One picture with CIIP units recorded and uploaded; the stages' frames are filled from the two results."""

    def __init__(self, dev, pic, d, order=None, d_mvf=None, ticket=None, guard=0):
        """d_mvf: the device MvField table the CIIP stage reads (by default the table painted from the units, uploaded).  ticket: the ticket
        order of the walk (by default the recorder's).  guard: rows of sentinel bytes kept above and below every plane."""
        k = self.k = pcs.Keep()
        self.dev, self.pic = dev, pic
        rec = dev.vvc355_rec_create()
        try:
            o = self.o = checked_record(dev, pic, d, rec=rec, order=order)
            self.d_arena = k.up(o.arena if o.arena_len else np.zeros(4, np.int32))
            assert dev.vvc355_rec_bind(rec, self.d_arena.ptr) == 0
            cmds = rk._copy(o.res.cmds, o.res.n_cmds, rk.CMD)
        finally:
            dev.vvc355_rec_destroy(rec)
        assert len(o.u.ciip) > 5 and o.u.totals["ciip_scratch_len"] > 0
        res, bd = o.res, pic.bd
        self.host_planes = [tc.pitched(p) for p in pic.planes]
        self.d_planes = [GuardedPlane(k, p, guard) for p in self.host_planes]
        self.ticket = o.order if ticket is None else np.ascontiguousarray(ticket, np.int32)
        assert ticket is None or (pcs.order_check(dev, o.ctus, pic.ncx, pic.ncy, self.ticket) == 0 and
                                  rc.order_defect(o.ctus, pic.ncx, pic.ncy, self.ticket) is None), "not launched"
        strides = self.strides = [p.shape[1] * pic.isz for p in self.host_planes]
        st, self.scaled, self.d_table, d_cmds, (d_slice, d_col, d_row) = recorded_stages(k, dev, pic, d, o, cmds, self.d_arena, self.d_planes, strides,
                                                                                        self.ticket)
        # the CIIP stage: the recorder's records, the SAME command array
        p = self.p = ciip_inputs(pic, o.u, cmds)
        self.dims, self.refs, self.lut = content(pic, p)
        d_ref = [[[k.up(batch.to_pitched(self.refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
        d_reft = k.up(np.frombuffer(bytes(cf.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], strides)), np.uint8))
        d_jobs = batch.DeviceBuffer(max(1, p.n_jobs) * cf.BIPRED_JOB_DT.itemsize)
        k.keep.append(d_jobs)
        d_scratch = k.up(np.zeros(p.scratch_len, pic.planes[0].dtype))
        d_sl, d_lut = k.up(np.frombuffer(bytes(p.slices), np.uint8)), k.up(self.lut)
        st["ciip"] = k.frame(p.frame(p.pic([b.ptr for b in self.d_planes], strides, (d_mvf if d_mvf is not None else k.up(p.mvf)).ptr, d_reft.ptr,
                                           d_sl.ptr, d_lut.ptr),
                                     k.up(p.cus).ptr, d_jobs.ptr, d_scratch.ptr, d_cmds.ptr, d_slice.ptr, d_col.ptr, d_row.ptr))
        self.d_reft, self.d_slices, self.d_lut, self.d_maps, self.strides = d_reft, d_sl, d_lut, (d_slice, d_col, d_row), strides
        self.stages = st

    def motion_stages(self, d_mvf, dmvr_ptr=0):
        """What runs ahead of the CIIP stage, from the recorder's lists: (the vvc355_mvf_unit_frame that fills d_mvf and the affine records'
        PROF fields — device address, host frame —, the stages `inter`, `affine`, `gpm` over this picture's planes).  dmvr_ptr: the device
        tab_dmvr_mvf table of the regular pass, or 0."""
        import affine_gpm_cases as agc
        pic, k, u = self.pic, self.k, self.o.u
        g = mu.Geo(pic.width, pic.height, pic.ctb_log2)
        d_aff = k.up(u.affine)
        mf = mu.unit_frame(g, k.up(u.mvf).ptr, len(u.mvf), k.up(u.first_mvf).ptr, d_mvf.ptr, g.tw, d_aff.ptr, len(u.affine))
        base = self.p.pic([b.ptr for b in self.d_planes], self.strides, d_mvf.ptr, self.d_reft.ptr, self.d_slices.ptr, self.d_lut.ptr)
        scratch = lambda nbytes: k.up(np.zeros(max(64, nbytes), np.uint8)).ptr               # noqa: E731
        n, na, ng = (u.totals[t] for t in ("n_inter_jobs", "n_affine_jobs", "n_gpm_jobs"))
        fi = abi.InterFrame.from_buffer_copy(bytes(base))
        fi.pus, fi.n_pus, fi.n_jobs, fi.dmvr_mvf = k.up(u.inter).ptr, len(u.inter), n, dmvr_ptr
        fi.jobs_luma, fi.jobs_chroma, fi.records = scratch(n * cf.BIPRED_JOB_DT.itemsize), scratch(2 * n * cf.BIPRED_JOB_DT.itemsize), scratch(32 * n)
        fa = abi.AffineFrame(pic=base, cus=d_aff.ptr, jobs_luma=scratch(na * agc.AFFINE_JOB_DT.itemsize),
                             jobs_chroma=scratch(2 * (na >> (pic.hs + pic.vs)) * cf.BIPRED_JOB_DT.itemsize), n_cus=len(u.affine), n_jobs=na)
        fg = abi.GpmFrame(pic=base, cus=k.up(u.gpm).ptr, jobs=scratch(ng * agc.GPM_JOB_DT.itemsize), n_cus=len(u.gpm), n_jobs=ng)
        assert len(u.inter) and len(u.affine) and len(u.gpm) and len(u.ciip)
        return k.frame(mf), dict(inter=k.frame(fi), affine=k.frame(fa), gpm=k.frame(fg))

    def run_entries(self):
        dev, st, bd = self.dev, self.stages, self.pic.bd
        call = lambda name, fn, *a: fn(None, st[name][0], ctypes.addressof(st[name][1]), *a) if name in st else 0      # noqa: E731
        assert dev.vvc355_ciip_frame_pass(None, bd, st["ciip"][0], ctypes.addressof(st["ciip"][1])) == 0
        assert call("intra_tb", dev.vvc355_intra_tb_pass) == 0
        if self.scaled:
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 1) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 1) == 0
            dev.vvc355_lmcs_vpdu_scale_pass(None, bd, st["lmcs_scale"][0], ctypes.addressof(st["lmcs_scale"][1]))
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 2) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 2) == 0
        else:
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 3) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 3) == 0
        dev.vvc355_recon_frame_pass(None, bd, st["recon"][0], ctypes.addressof(st["recon"][1]))

    def result(self):
        self.dev.vvc355_stream_sync(None)
        assert self.dev.vvc355_last_error() == 0
        planes = [b.to_host(h.dtype, h.shape) for b, h in zip(self.d_planes, self.host_planes)]
        for c, (g, h, p) in enumerate(zip(planes, self.host_planes, self.pic.planes)):
            assert np.array_equal(g[:, p.shape[1]:], h[:, p.shape[1]:]), f"component {c}: the pitch padding was written"
        return [g[:, :p.shape[1]] for g, p in zip(planes, self.pic.planes)]


def ciip_oracle(orc, pic, d, e, refs, lut, dims, start=None, whole=False, jobs_hook=None, cmds_hook=None, scale_table=None):
    """The chained oracle: the inter parts of the CIIP units (orc_bipred_block on the expected jobs, unblended chroma straight onto the
    planes), then ref_recon_cases.oracle_side on those planes with the CIIP commands completed as the builder completes them.
    whole: return (planes, scale table or None) instead of the planes.  jobs_hook(p, jobs) changes the expected jobs in place,
    cmds_hook(p, d2) replaces d2.cmds (and d2.ctus) of this call's own copy of d after the commands are completed, scale_table replaces
    the table of oracle_side: the sensitivity checks of
    tests/ref_picture_cases.py apply a misreading there."""
    planes = [np.ascontiguousarray(p).copy() for p in (start or pic.planes)]
    p = ciip_inputs(pic, e, d.cmds)
    scratch = np.zeros(p.scratch_len, planes[0].dtype)
    jobs = cf.expect_jobs(p, lambda c: (planes[c].ctypes.data, dims[c][0] * pic.isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * pic.isz),
                          scratch.ctypes.data, lut.ctypes.data)
    assert (jobs["w"] > 0).all(), "a CIIP record the builder would reject"
    if jobs_hook is not None:
        jobs_hook(p, jobs)
    cf.call(orc.orc_bipred_block, pic.bd, jobs)
    d2, pic2 = SimpleNamespace(**vars(d)), SimpleNamespace(**vars(pic))
    pic2.planes = planes
    d2.pic, d2.cmds = pic2, cf.expect_cmds(p, scratch.ctypes.data)
    is_ciip = d2.cmds["kind"] == abi.RECON_CIIP
    assert is_ciip.sum() >= len(p.cus) and d2.cmds["resid"][is_ciip].all() and d2.cmds["joint"][is_ciip].all()
    if cmds_hook is not None:
        cmds_hook(p, d2)
    out, table, _arena = rc.oracle_side(orc, d2, scale_table)
    return (out, table) if whole else out


def gpm_golden():
    return np.load(os.path.join(rc.ROOT, "tests", "golden", "gpm_tables.npz"))


def inter_oracle(orc, pic, e, mvf, aff, refs, lut, dims, slices, planes, dmvr=None):
    """The three kinds of inter units that predict onto the picture, on host planes in place: orc_inter_frame_pass on the vvc355_inter_pu
    list, then pred_affine_blk / pred_gpm_blk as affine_gpm_cases restates them, through the oracle's block functions.  dmvr: the
    tab_dmvr_mvf table (a copy of mvf) the regular pass writes the refined motion to."""
    import affine_gpm_cases as agc
    isz, bd = pic.isz, pic.bd
    strides = [dm[0] * isz for dm in dims]
    reft = cf.ref_table([[[refs[l][r][c].ctypes.data for c in range(3)] for r in range(2)] for l in range(2)], strides)
    plane = lambda c: (planes[c].ctypes.data, strides[c])                                # noqa: E731
    ref = lambda l, r, c: (refs[l][r][c].ctypes.data, strides[c])                        # noqa: E731
    n = e.totals["n_inter_jobs"]
    jl, jc, recs = np.zeros(max(1, n), cf.BIPRED_JOB_DT), np.zeros(max(1, 2 * n), cf.BIPRED_JOB_DT), np.zeros((max(1, n), 8), np.int32)
    pus = np.ascontiguousarray(e.inter)
    f = abi.InterFrame()
    for c in range(3):
        f.dst[c], f.dst_stride[c] = plane(c)
    f.mvf, f.refs, f.pus, f.slices = mvf.ctypes.data, ctypes.addressof(reft), pus.ctypes.data, ctypes.addressof(slices)
    f.jobs_luma, f.jobs_chroma, f.records, f.lmcs_fwd_lut = jl.ctypes.data, jc.ctypes.data, recs.ctypes.data, lut.ctypes.data
    f.dmvr_mvf = dmvr.ctypes.data if dmvr is not None else 0
    f.mvf_stride, f.n_pus, f.n_jobs, f.width, f.height = pic.width // 4, len(pus), n, pic.width, pic.height
    f.hs, f.vs, f.chroma_format_idc, f.pixel_shift = pic.hs, pic.vs, pic.idc, int(isz == 2)
    orc.orc_inter_frame_pass.argtypes, orc.orc_inter_frame_pass.restype = [ctypes.c_int, ctypes.POINTER(abi.InterFrame)], None
    orc.orc_inter_frame_pass(bd, ctypes.byref(f))
    w = agc.AffineGpmWork.__new__(agc.AffineGpmWork)
    w.width, w.height, w.hs, w.vs, w.chroma, w.isz, w.mvf, w.slices = pic.width, pic.height, pic.hs, pic.vs, pic.idc != 0, isz, mvf, slices
    w.aff, w.n_aff_jobs = aff.view(agc.AFFINE_CU_DT), e.totals["n_affine_jobs"]
    w.gpm, w.n_gpm_jobs = np.ascontiguousarray(e.gpm).view(agc.GPM_CU_DT), e.totals["n_gpm_jobs"]
    golden = gpm_golden()
    masks = np.ascontiguousarray(golden["ff_vvc_gpm_weights"])
    a_l, a_c = w.expect_affine(plane, ref, lambda u: w.aff.ctypes.data + u * agc.AFFINE_CU_DT.itemsize, lut.ctypes.data)
    g = w.expect_gpm(plane, ref, lut.ctypes.data, masks.ctypes.data, golden)
    agc.call(orc.orc_affine_block, bd, a_l)
    agc.call(orc.orc_bipred_block, bd, a_c)
    agc.call(orc.orc_gpm_block, bd, g)
    return planes



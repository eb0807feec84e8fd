"""GPU: vvc355_picture_pass and what came with it.

1. vvc355_lmcs_frame_pass alone against a numpy LUT lookup and against vvc355_lmcs_batch on per-CTB jobs, the pitch padding and the
   untouched CTBs compared whole;
2. the filter half: the pictures of ref_pass_cases through one picture (tab_fill for the motion, bs_rec, qp_rec, both deblocking directions,
   SAO, the ALF build and filter) to the reference's digests in tests/golden/ref_passes.json;
3. the reconstruction half: ciip_frame_cases.e2e_work() through CIIP build + predict, RECON (host order tables given) and inverse LMCS
   against the oracle's reconstruction followed by the numpy LUT;
4. the TB order: both TB record passes around the scale pass on an LMCS picture, against the oracle walk, and the single-call path;
6. a reference wait across two streams; 7. graph capture; 8. build + _predict equals _pass for the four inter drivers.
5. one picture through both halves: the picture of (3) with unit records derived from its units, through the whole order, against the
   chained oracle passes."""
import ctypes

import numpy as np
import pytest

import bipred_cases as bc
import bs_rec_cases as rc
import ciip_frame_cases as cc
import inter_frame_cases as ifc
import inter_tb_cases as tc
import picture_cases as pcs
import qp_rec_cases as qc
import ref_pass_cases as pc
import ts_tb_cases as ts
from ffvvc_amd import abi, batch
from test_ref_passes_gpu import Device, _download, _hold, _locate_deblock, _output_tables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


# ---------------------------------------------------------------------------------------------------------------- 1. inverse LMCS alone

LMCS_ALIGNED = [True, True, True, False]


@pytest.mark.parametrize("case", range(len(pcs.LMCS_CASES)))
def test_lmcs_frame_pass(dev, case):
    c = pcs.lmcs_case(case)
    k = pcs.Keep()
    image = pcs.lmcs_bytes(c, c.plane)
    want = pcs.lmcs_bytes(c, pcs.lmcs_expected(c))
    inside = c.width * c.isz
    assert (want[:, :inside] != image[:, :inside]).mean() > 0.3 and np.array_equal(want[:, inside:], image[:, inside:])
    assert np.any(want[:, :inside] == image[:, :inside], axis=1).all()                  # CTBs that stay as they are, in every row
    d_lut, d_slice, d_used = k.up(c.lut), k.up(c.slice_idx), k.up(c.used)
    d_a, d_b = k.up(image), k.up(image)
    assert d_a.ptr % 16 == 0 and (c.pitch % 16 == 0) == LMCS_ALIGNED[case]          # which path the rows take
    dev_ptr, f = k.frame(pcs.lmcs_frame(c, d_a.ptr, d_lut.ptr, d_slice.ptr, d_used.ptr))
    assert dev.vvc355_lmcs_frame_pass(None, c.bd, dev_ptr, ctypes.addressof(f)) == 0
    jobs = pcs.lmcs_jobs(c, d_b.ptr, d_lut.ptr)
    d_jobs = k.up(jobs)
    dev.vvc355_lmcs_batch(None, c.bd, d_jobs.ptr, len(jobs), 1 << c.ctb_log2, 1 << c.ctb_log2)
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    got, old = d_a.to_host(np.uint8, image.shape), d_b.to_host(np.uint8, image.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"case {case}: {len(bad)} bytes differ from the numpy lookup, first at (row, byte) {bad[0].tolist()}"
    assert np.array_equal(old, want), "vvc355_lmcs_batch on per-CTB jobs differs from the numpy lookup"


# ---------------------------------------------------------------------------------------------------------------- 2. the filter half

def _stage(d, f):
    """A stage of picture_cases.picture(): the frame uploaded, and the host frame itself."""
    return d.frame(f)[0], f


def _record_stages(d, pic, plane_bufs, pitched, mvf=None):
    """tab_fill (motion only), bs_rec, qp_rec and both deblocking directions of `pic` on `plane_bufs`: (stages, tables).  mvf: the device
    MvField table to fill (a fresh one by default)."""
    t, p = pic.t, pic.rec
    (cu, cu_first), (tu, tu_first), (mv, mv_first) = rc.grouped(t)
    chroma = pic.n_comp == 3
    tabs = _output_tables(d, pic)
    for n in rc.TB_C + qc.TABLES:
        tabs[n] = d.up(np.full((t.th, t.tw), 0xEE, np.uint8))
    tabs["mvf"] = mvf if mvf is not None else batch.DeviceBuffer(t.mvf.nbytes)
    for n in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
        tabs[n] = d.up(getattr(t, n))
    tabs["dbp"] = d.up(pic.arrays["dbp"])
    addr = lambda n: tabs[n].ptr          # noqa: E731
    d_cu, d_cu_first, d_tu, d_tu_first, d_cu_qp, d_tu_qp_c, d_mv, d_mv_first = (d.up(a) for a in (cu, cu_first, tu, tu_first, p.cu_qp, p.tu_qp_c, mv, mv_first))
    cu_arg, tu_arg = (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr)
    strides = [q.strides[0] for q in pitched]
    stages = dict(
        tab_fill=_stage(d, t.fill_frame(0, 0, d_mv.ptr, (0, 0, len(mv)), lambda name: tabs["mvf"].ptr if name == "mvf" else 0, (0, 0, d_mv_first.ptr))),
        bs_rec=_stage(d, rc.rec_frame(t, cu_arg, tu_arg, addr, pic.n_comp, tb_c=chroma)),
        qp_rec=_stage(d, qc.qp_frame(t, cu_arg, tu_arg if chroma else (0, 0, 0), d_cu_qp.ptr, d_tu_qp_c.ptr if chroma else 0,
                                     [tabs[n].ptr if chroma or n == "qp_y" else 0 for n in qc.TABLES], t.tw, pic.n_comp)),
        deblock_v=_stage(d, pc.deblock_frame(pic, 1, [b.ptr for b in plane_bufs], strides, addr)),
        deblock_h=_stage(d, pc.deblock_frame(pic, 0, [b.ptr for b in plane_bufs], strides, addr)))
    return stages, tabs


def _filter_stages(d, fp, src_bufs, pitched, which=("sao", "alf")):
    """SAO from src_bufs into fresh planes, ALF from those (or from src_bufs without SAO) into fresh planes: (stages, alf_work, outputs)."""
    t = fp.t
    tabs = {"sao": d.up(fp.sao), "alf": d.up(fp.alf), "slice_idx": d.up(t.slice_idx), "col_bd": d.up(t.col_bd), "row_bd": d.up(t.row_bd)}
    tabs["slices"] = d.up(np.frombuffer(bytes(pc.alf_slices(fp, [d.up(a).ptr for a in fp.aps])), np.uint8))
    strides = [q.strides[0] for q in pitched]
    stages, out, work, src = {}, {}, 0, src_bufs
    for s in which:
        out_pitched = [np.full_like(q, 0x21) for q in pitched]
        out_bufs = [d.up(q) for q in out_pitched]
        make = pc.sao_frame if s == "sao" else pc.alf_frame
        stages[s] = _stage(d, make(fp, [b.ptr for b in out_bufs], [b.ptr for b in src], strides, strides, lambda n: tabs[n].ptr))
        out[s] = (out_bufs, out_pitched)
        if s == "alf":
            work = d.up(np.zeros(d.dev.vvc355_alf_frame_work_bytes(t.cw * t.ch), np.uint8)).ptr
        src = out_bufs
    return stages, work, out


@pytest.mark.parametrize("name", pc.REC_PATH)
def test_deblocking_half_from_records(dev, orc, golden, name):
    """One picture: motion table, boundary strengths, QP tables, vertical then horizontal edges.  (A second picture with the vertical
    stage alone on fresh planes, reading the tables the first left, gives the planes between the two.)"""
    pic = pc.deblock_picture(orc, name)
    d, t = Device(dev), pic.t
    pitched, bufs = d.planes(pic.planes)
    stages, tabs = _record_stages(d, pic, bufs, pitched)
    assert pcs.run(dev, None, pic.bd, pcs.picture(stages)) == 0
    d.sync()
    assert dev.vvc355_last_error() == 0
    got = {n: tabs[n].to_host(np.uint8, (t.th, t.tw)) for n in t.OUT}
    got["h"] = _download(bufs, pitched, pic.planes)
    pitched_v, bufs_v = d.planes(pic.planes)
    fv = pc.deblock_frame(pic, 1, [b.ptr for b in bufs_v], [q.strides[0] for q in pitched_v], lambda n: tabs[n].ptr)
    assert pcs.run(dev, None, pic.bd, pcs.picture(dict(deblock_v=_stage(d, fv)))) == 0
    d.sync()
    got["v"] = _download(bufs_v, pitched_v, pic.planes)
    _hold(name, golden[name], got, ("v", "h"), t.OUT, lambda: _locate_deblock(orc, pic, got))


@pytest.mark.parametrize("name", pc.FILTER)
def test_sao_and_alf_through_the_picture(dev, orc, golden, name):
    fp = pc.filter_picture(name)
    got = {}
    for s in ("sao", "alf"):
        d = Device(dev)
        pitched, bufs = d.planes(fp.planes)
        stages, work, out = _filter_stages(d, fp, bufs, pitched, (s,))
        assert pcs.run(dev, None, fp.bd, pcs.picture(stages, alf_work=work)) == 0
        d.sync()
        got[s] = _download(*out[s], fp.planes)
    assert dev.vvc355_last_error() == 0
    _hold(name, golden[name], got, ("sao", "alf"), (),
          lambda: sum((pc.plane_differences(name, s, pc.run_filter(orc, "orc", fp, s), got[s], label="oracle") for s in ("sao", "alf")), []))


def test_whole_filter_chain_in_one_picture(dev, orc, golden):
    """C0: every filter stage of the order in ONE call, each on what the previous one left in device memory."""
    dp, fp = pc.chain_picture()
    d, t = Device(dev), dp.t
    pitched, bufs = d.planes(dp.planes)
    stages, tabs = _record_stages(d, dp, bufs, pitched)
    more, work, out = _filter_stages(d, fp, bufs, pitched)
    stages.update(more)
    assert pcs.run(dev, None, dp.bd, pcs.picture(stages, alf_work=work)) == 0
    d.sync()
    assert dev.vvc355_last_error() == 0
    got = {n: tabs[n].to_host(np.uint8, (t.th, t.tw)) for n in t.OUT}
    got["h"] = _download(bufs, pitched, dp.planes)
    got["sao"], got["alf"] = (_download(*out[s], dp.planes) for s in ("sao", "alf"))

    def locate():
        want = pc.run_chain(orc, "orc")
        lines = pc.table_differences(dp, want, got, label="oracle")
        for s in ("h", "sao", "alf"):
            lines += pc.plane_differences(pc.CHAIN, s, want[s], got[s], label="oracle")
        return lines
    rec = pc.stage_digests(got, ("h", "sao", "alf"), t.OUT)          # the planes between the two directions are not kept by one call
    bad = [k for k in rec if rec[k] != golden[pc.CHAIN][k]]
    assert not bad, f"{pc.CHAIN}: {bad} do not hash to the reference's digests\n" + "\n".join(locate())


# ---------------------------------------------------------------------------------------------------------------- 3. the reconstruction half

@pytest.fixture(scope="module")
def recon_picture(dev, orc):
    return pcs.ReconPicture(dev, orc)


def _assert_planes(got, want, what):
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"


def test_reconstruction_half(dev, recon_picture):
    rp = recon_picture
    rp.reset()
    assert sorted(rp.order.tolist()) == rp.raster.tolist()                         # the critical-path order, checked on the host first
    pic = pcs.picture(rp.stages(), recon_tables=rp.tables())
    assert pcs.run(dev, None, rp.bd, pic) == 0
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    _assert_planes(rp.planes(), rp.want, "CIIP + RECON + inverse LMCS")
    assert np.any(rp.want[0] != rp.recon[0]) and sum(int((w != s).sum()) for w, s in zip(rp.recon, rp.start)) > 256 * 192 // 4
    # a ticket order that would hang the pass is refused on the host: nothing runs, the planes stay as they are
    rp.reset()
    bad = rp.order.copy()
    at = {int(rs): i for i, rs in enumerate(bad)}
    rs = next(int(r) for r in bad if pcs.waits_for(rp.work.ctus, rp.work.ncx, r))
    dep = pcs.waits_for(rp.work.ctus, rp.work.ncx, rs)[0]
    bad[at[rs]], bad[at[dep]] = dep, rs
    ret = pcs.run(dev, None, rp.bd, pcs.picture(rp.stages(), recon_tables=(rp.work.ctus, bad)))
    assert pcs.decode(ret) == (abi.PIC_STAGE_RECON_ORDER, abi.RECON_ORDER_E_DEPENDENCY)
    dev.vvc355_stream_sync(None)
    _assert_planes(rp.planes(), rp.start, "a refused picture")


def test_one_picture_through_both_halves(dev, orc, recon_picture):
    """5. The reconstruction picture with coding-unit, transform-unit and motion records derived from its own units, drawn QPs and per-CTB
    SAO / ALF parameters, through the whole order in one call: the MvField table the CIIP builder reads is the one tab_fill writes from the
    motion records (the table is garbage before the call), the filters run on what RECON and inverse LMCS left.  Against the chained oracle
    passes on the oracle's reconstruction."""
    rp = recon_picture
    dp, fp = pcs.whole_picture(rp)
    rp.reset()
    d, t = Device(dev), dp.t
    garbage = np.full(rp.p.mvf.nbytes, 0xEE, np.uint8)
    dev.vvc355_upload(rp.d_mvf.ptr, garbage.ctypes.data, garbage.nbytes)
    try:
        stages, tabs = _record_stages(d, dp, rp.d_planes, rp.pitched, mvf=rp.d_mvf)
        more, work, out = _filter_stages(d, fp, rp.d_planes, rp.pitched)
        stages.update(more)
        stages.update(rp.stages())
        assert set(stages) == {"tab_fill", "ciip", "bs_rec", "qp_rec", "alf", "recon", "lmcs", "deblock_v", "deblock_h", "sao"}
        assert pcs.run(dev, None, rp.bd, pcs.picture(stages, alf_work=work, recon_tables=rp.tables())) == 0
        d.sync()
        assert dev.vvc355_last_error() == 0
        got = {n: tabs[n].to_host(np.uint8, (t.th, t.tw)) for n in t.OUT}
        got["h"] = rp.planes()
        got["sao"], got["alf"] = (_download(*out[s], rp.want) for s in ("sao", "alf"))
    finally:
        m = np.ascontiguousarray(rp.p.mvf)
        dev.vvc355_upload(rp.d_mvf.ptr, m.ctypes.data, m.nbytes)
    want = pc.run_deblock(orc, "orc", dp)                       # dp.planes = the oracle's reconstruction + the numpy LUT
    want["sao"] = pc.run_filter(orc, "orc", fp, "sao", want["h"])
    want["alf"] = pc.run_filter(orc, "orc", fp, "alf", want["sao"])
    lines = pc.table_differences(dp, want, got, label="oracle")
    for s in ("h", "sao", "alf"):
        lines += pc.plane_differences("both halves", s, want[s], got[s], label="oracle")
    assert not lines, "\n".join(lines)
    assert all(np.any(a != b) for a, b in zip(want["h"], rp.want)) and all(np.any(a != b) for a, b in zip(want["alf"], want["sao"]))


# ---------------------------------------------------------------------------------------------------------------- 4. the TB order

def _tb_specs(rng, pic, scaled):
    inter, skip = [], []
    for c_idx in range(3):
        for k, cell in enumerate(ts.cells(pic, c_idx)):
            lw, lh = [(2, 2), (3, 3), (4, 4), (5, 5), (3, 4), (5, 2)][(k + c_idx) % 6] if c_idx == 0 else [(1, 3), (3, 3), (4, 4), (2, 1)][(k + c_idx) % 4]
            x, y = ts.in_cell(rng, cell, lw, lh)
            joint = 8 if (scaled and c_idx and (1 << lw) * (1 << lh) > 4) else 0
            if (k + c_idx) % 2:
                inter.append(tc.random_spec(rng, c_idx, x, y, lw, lh, keep=k % 5 == 4, joint=joint))
            else:
                skip.append(ts.random_spec(rng, c_idx, x, y, lw, lh, bdpcm=k % 4 == 0, vert=bool(k & 2), keep=k % 5 == 2, joint=joint))
    return inter, skip


@pytest.mark.parametrize("lmcs", [True, False])
def test_tb_passes_around_the_scale_pass(dev, orc, lmcs):
    """With a lmcs_scale stage: inter_tb(1), ts_tb(1), the scale table from the luma those reconstructed, inter_tb(2), ts_tb(2) with the
    chroma residuals scaled through the table; without one, each pass once with both channel types."""
    tc.bind_oracle(orc)
    bd, W, H = 10, 256, 128                      # 2 x 4 units of 64: 16 chroma blocks, enough scaled ones among them
    rng = np.random.default_rng(0x5EED7AA0 + lmcs)
    if lmcs:
        import recon_cases
        planes = [tc.unit_dc_luma(rng, bd, W, H, 64)] + [rng.integers(0, 1 << bd, size=(H >> 1, W >> 1), dtype=np.int64).astype(np.uint16) for _ in range(2)]
        pic = tc.Picture(planes, bd, model=recon_cases.ReconWork.lmcs_model(rng, bd))
    else:
        pic = tc.Picture.random(rng, bd, W, H)
    inter, skip = _tb_specs(rng, pic, lmcs)
    inter, bin_first = tc.group(inter)
    skip, class_first = ts.group(skip)
    assert len(inter) >= 5 and len(skip) >= 5
    both = inter + skip
    offs, n = tc.arena_offsets(both)
    arena0 = tc.start_arena(both, offs, n, None)
    want_planes, want_arena, want_table = ts.oracle_walk(orc, pic, both, offs, arena0)
    f_i = tc.Frame(pic, inter, bin_first, offs[:len(inter)], arena0, 15, None)
    f_t = ts.Frame(pic, skip, class_first, offs[len(inter):], arena0, 15, None, shared=f_i)
    f_i.reset(dev)
    stages = dict(inter_tb=(f_i.d_f.ptr, f_i.f), ts_tb=(f_t.d_f.ptr, f_t.f))
    if lmcs:
        stages["lmcs_scale"] = (f_i.dpic.d_sf.ptr, f_i.dpic.sf)
        assert f_i.f.scale_table == f_t.f.scale_table == f_i.dpic.sf.scale != 0
        assert sum(1 for s in both if s["joint"] & 8 and not s["keep"]) > 5
    assert pcs.run(dev, None, bd, pcs.picture(stages)) == 0
    got = f_i.dpic.pitched_planes(dev)
    assert dev.vvc355_last_error() == 0
    for c, (g, w) in enumerate(zip(got, f_i.dpic.expected_pitched(want_planes))):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"
    assert np.array_equal(f_i.arena(dev), want_arena)
    if lmcs:
        assert np.array_equal(f_i.dpic.d_table.to_host(np.int16, want_table.shape), want_table)
        # without the scale stage the same frames are refused as a whole
        ret = pcs.run(dev, None, bd, pcs.picture({k: v for k, v in stages.items() if k != "lmcs_scale"}))
        assert pcs.decode(ret) == (abi.PIC_STAGE_PICTURE, abi.PIC_E_SCALE_TABLE)
    assert any(np.any(w != p) for w, p in zip(want_planes, pic.planes))


# ---------------------------------------------------------------------------------------------------------------- 6. / 8. inter pictures

class InterPicture:
    """An inter_frame_cases picture on the device; refs[0][0] luma may be a caller's device plane (pitch of the 256-byte rule)."""

    def __init__(self, dev, rng, bd, w, h, ref00_luma=None):
        self.dev, self.bd, self.k = dev, bd, pcs.Keep()
        k, hs, vs, isz = self.k, 1, 1, 2
        self.dims = dims = [(w, h), (w >> hs, h >> vs), (w >> hs, h >> vs)]
        self.work = work = ifc.InterWork(rng, w, h)
        base = [bc.smooth_picture(rng, ph, pw, bd) for (pw, ph) in dims]
        self.refs = refs = [[[bc.shifted(base[c], (2 * l - 1) * (r + 1) >> (hs if c else 0), (1 - 2 * l) * (r + 2) >> (vs if c else 0)) for c in range(3)]
                             for r in range(2)] for l in range(2)]
        if ref00_luma is not None:
            refs[0][0][0] = ref00_luma[0]
        self.lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)
        self.jl_dt = batch.job_array(abi.BipredJob, 1).dtype
        self.pitches = pitches = [batch.plane_pitch(d[0], isz) for d in dims]
        d_ref = [[[k.up(batch.to_pitched(refs[l][r][c])).ptr for c in range(3)] for r in range(2)] for l in range(2)]
        if ref00_luma is not None:
            d_ref[0][0][0] = ref00_luma[1]
        t = cc.ref_table(d_ref, pitches)
        self.zero = [batch.to_pitched(np.zeros((ph, pw), base[0].dtype)) for (pw, ph) in dims]
        self.d_dst = [k.up(z) for z in self.zero]
        self.d_jl, self.d_jc, self.d_rec = k.up(np.zeros(work.n_jobs, self.jl_dt)), k.up(np.zeros(2 * work.n_jobs, self.jl_dt)), k.up(np.zeros((work.n_jobs, 8), np.int32))
        self.d_dmvr = k.up(work.mvf)
        self.f = work.frame([b.ptr for b in self.d_dst], pitches, k.up(work.mvf).ptr, k.up(np.frombuffer(bytes(t), np.uint8)).ptr, k.up(work.pus).ptr,
                            k.up(np.frombuffer(bytes(work.slices), np.uint8)).ptr, self.d_jl.ptr, self.d_jc.ptr, self.d_rec.ptr, hs, vs, isz,
                            dmvr_ptr=self.d_dmvr.ptr, lut_ptr=k.up(self.lut).ptr)
        self.d_f = k.up(np.frombuffer(bytes(self.f), np.uint8))

    def oracle(self, orc):
        orc.orc_inter_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.InterFrame)]
        orc.orc_inter_frame_pass.restype = None
        work, dims, refs, isz = self.work, self.dims, self.refs, 2
        want = [np.zeros((ph, pw), refs[0][0][0].dtype) for (pw, ph) in dims]
        h_jl, h_jc, h_rec, h_dmvr = np.zeros(work.n_jobs, self.jl_dt), np.zeros(2 * work.n_jobs, self.jl_dt), np.zeros((work.n_jobs, 8), np.int32), work.mvf.copy()
        self._hold = [np.ascontiguousarray(refs[l][r][c]) for l in range(2) for r in range(2) for c in range(3)]
        t = cc.ref_table([[[self._hold[(l * 2 + r) * 3 + c].ctypes.data for c in range(3)] for r in range(2)] for l in range(2)], [d[0] * isz for d in dims])
        hf = work.frame([p.ctypes.data for p in want], [d[0] * isz for d in dims], work.mvf.ctypes.data, ctypes.addressof(t), work.pus.ctypes.data,
                        ctypes.addressof(work.slices), h_jl.ctypes.data, h_jc.ctypes.data, h_rec.ctypes.data, 1, 1, isz, dmvr_ptr=h_dmvr.ctypes.data, lut_ptr=self.lut.ctypes.data)
        orc.orc_inter_frame_pass(self.bd, ctypes.byref(hf))
        return want

    def reset(self):
        for b, z in zip(self.d_dst, self.zero):
            self.dev.vvc355_upload(b.ptr, z.ctypes.data, z.nbytes)
        for b in (self.d_jl, self.d_jc, self.d_rec):
            z = np.zeros(b.nbytes, np.uint8)
            self.dev.vvc355_upload(b.ptr, z.ctypes.data, z.nbytes)
        m = np.ascontiguousarray(self.work.mvf)
        self.dev.vvc355_upload(self.d_dmvr.ptr, m.ctypes.data, m.nbytes)

    def outputs(self):
        return [b.to_host(np.uint8, (b.nbytes,)) for b in self.d_dst + [self.d_jl, self.d_jc, self.d_rec, self.d_dmvr]]

    def planes(self):
        return [b.to_host(z.dtype, z.shape)[:, :d[0]] for b, z, d in zip(self.d_dst, self.zero, self.dims)]


def test_picture_waits_for_its_reference_picture(dev, orc):
    """Picture A: inverse LMCS of a luma plane on stream 1, `done` = evA.  Picture B: inter prediction from A's plane on stream 2 with
    refs = [evA].  B is the oracle's prediction from the MAPPED plane; both `done` events are reported after the synchronisation."""
    bd, w, h = 10, 128, 64
    rng = np.random.default_rng(pcs.SEED + 600)
    k = pcs.Keep()
    plane = bc.smooth_picture(rng, h, w, bd)
    inv = np.random.default_rng(pcs.SEED + 601).permutation(1 << bd).astype(plane.dtype)
    c = pcs.SimpleNamespace(bd=bd, width=w, height=h, ctb_log2=6, cw=2, ch=1, pitch=batch.plane_pitch(w, 2), n_slices=2, isz=2,
                            slice_idx=np.array([0, 1], np.int16), used=np.array([1, 0], np.uint8), lut=inv, plane=plane)
    mapped = pcs.lmcs_expected(c)
    assert np.any(mapped != plane)
    d_plane = k.up(batch.to_pitched(plane))
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_plane.ptr, k.up(inv).ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))
    b = InterPicture(dev, rng, bd, w, h, ref00_luma=(mapped, d_plane.ptr))
    want = b.oracle(orc)
    s1, s2 = dev.vvc355_stream_create(), dev.vvc355_stream_create()
    ev_a, ev_b = dev.vvc355_event_create(), dev.vvc355_event_create()
    try:
        assert pcs.run(dev, s1, bd, pcs.picture(dict(lmcs=(lf_ptr, lf)), done=ev_a)) == 0
        assert pcs.run(dev, s2, bd, pcs.picture(dict(inter=(b.d_f.ptr, b.f)), refs=[ev_a], done=ev_b)) == 0
        dev.vvc355_stream_sync(s2)
        assert dev.vvc355_event_query(ev_b) == 1 and dev.vvc355_event_query(ev_a) == 1
        dev.vvc355_stream_sync(s1)
        assert dev.vvc355_last_error() == 0
        got_a = d_plane.to_host(plane.dtype, (h, c.pitch // 2))[:, :w]
        assert np.array_equal(got_a, mapped)
        _assert_planes(b.planes(), want, "prediction from the mapped reference")
    finally:
        for ev in (ev_a, ev_b):
            dev.vvc355_event_destroy(ev)
        for s in (s1, s2):
            dev.vvc355_stream_destroy(s)


def test_picture_captured_in_a_graph(dev, recon_picture):
    """The reconstruction half recorded once and replayed twice on restored inputs; a picture with a reference is refused while the stream
    captures, and leaves nothing in the graph."""
    rp = recon_picture
    rp.reset()
    s = dev.vvc355_stream_create()
    ev = dev.vvc355_event_create()
    try:
        dev.vvc355_graph_begin(s)
        for kw in (dict(refs=[ev]), dict(done=ev)):
            ret = pcs.run(dev, s, rp.bd, pcs.picture(rp.stages(), recon_tables=rp.tables(), **kw))
            assert pcs.decode(ret) == (abi.PIC_STAGE_PICTURE, abi.PIC_E_CAPTURE), kw
        ret = pcs.run(dev, s, rp.bd, pcs.picture(rp.stages(), recon_tables=rp.tables()))
        g = dev.vvc355_graph_end(s)
        assert ret == 0
        dev.vvc355_stream_sync(s)
        _assert_planes(rp.planes(), rp.start, "recorded, not run")
        for rep in range(2):
            rp.reset()
            dev.vvc355_graph_launch(g, s)
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
            _assert_planes(rp.planes(), rp.want, f"replay {rep}")
        dev.vvc355_graph_destroy(g)
    finally:
        dev.vvc355_event_destroy(ev)
        dev.vvc355_stream_destroy(s)


def test_inter_build_plus_predict_equals_pass(dev):
    p = InterPicture(dev, np.random.default_rng(pcs.SEED + 800), 10, 128, 128)
    args = (p.d_f.ptr, ctypes.addressof(p.f))
    dev.vvc355_inter_frame_pass(None, 10, *args)
    dev.vvc355_stream_sync(None)
    whole = p.outputs()
    p.reset()
    dev.vvc355_inter_frame_build(None, *args)
    dev.vvc355_inter_frame_predict(None, 10, *args)
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    halves = p.outputs()
    assert all(np.array_equal(a, b) for a, b in zip(whole, halves)) and whole[0].any() and whole[-1].any()


def test_ciip_build_plus_predict_equals_pass(dev):
    case = 0
    bd = cc.CASES[case][0]
    p = cc.case_picture(case)
    dims, refs, lut = cc.pictures(np.random.default_rng(0xC11B + case), p, bd)
    sentinel = (1 << bd) // 3
    a, b = (cc.DeviceRun(dev, p, bd, dims, refs, lut, sentinel) for _ in range(2))
    assert a.run() == 0
    assert dev.vvc355_ciip_frame_build(None, b.d_frame.ptr, ctypes.addressof(b.frame)) == 0
    assert dev.vvc355_ciip_frame_predict(None, bd, b.d_frame.ptr, ctypes.addressof(b.frame)) == 0
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    assert np.array_equal(a.scratch(), b.scratch()) and np.any(a.scratch() != sentinel)
    for c in range(3):
        assert np.array_equal(a.plane(c), b.plane(c))
    ca, cb = a.cmds(), b.cmds()
    patched = ca["resid"] != p.cmds["resid"]
    assert patched.any() and np.array_equal(ca["joint"], cb["joint"])
    assert np.array_equal(ca["resid"][patched] - a.d_scratch.ptr, cb["resid"][patched] - b.d_scratch.ptr) and np.array_equal(ca["resid"][~patched], cb["resid"][~patched])
    # the jobs: everything but the addresses, which are the two runs' own buffers
    ja, jb = a.jobs(), b.jobs()
    for name in ja.dtype.names:
        if name not in ("dst", "ref0", "ref1", "rec", "lmcs_lut"):
            assert np.array_equal(ja[name], jb[name]), name
    # a frame the pass refuses is refused by the predict half alike
    b.frame.ctb_log2 = 4
    assert dev.vvc355_ciip_frame_predict(None, bd, b.d_frame.ptr, ctypes.addressof(b.frame)) == abi.CIIP_E_CTB


def test_affine_and_gpm_build_plus_predict_equals_pass(dev):
    import affine_gpm_cases as agc
    bd, hs, vs, w, h, isz = 10, 1, 1, 256, 192, 2
    rng = np.random.default_rng(0xAF6 + 8)
    k = pcs.Keep()
    dims = [(w, h)] + [(w >> hs, h >> vs)] * 2
    work = agc.AffineGpmWork(rng, w, h, hs, vs, True, isz)
    base = [bc.smooth_picture(rng, ph, pw, bd) for (pw, ph) in dims]
    refs = [[[bc.shifted(base[c], (2 * l - 1) * (r + 1) >> (hs if c else 0), (1 - 2 * l) * (r + 2) >> (vs if c else 0)) for c in range(3)] for r in range(2)] for l in range(2)]
    lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)
    pitches = [batch.plane_pitch(d[0], isz) for d in dims]
    start = [batch.to_pitched(np.full((ph, pw), (1 << bd) // 3, base[0].dtype)) for (pw, ph) in dims]
    d_dst = [k.up(s) for s in start]
    d_ref = [[[k.up(batch.to_pitched(refs[l][r][c])).ptr for c in range(3)] for r in range(2)] for l in range(2)]
    t_refs = agc.ref_table(d_ref, [[pitches] * 2] * 2)
    n_c = 2 * (work.n_aff_jobs >> (hs + vs))
    sizes = (work.n_aff_jobs * agc.AFFINE_JOB_DT.itemsize, n_c * agc.BIPRED_JOB_DT.itemsize, work.n_gpm_jobs * agc.GPM_JOB_DT.itemsize)
    d_jl, d_jc, d_g = (k.up(np.zeros(n, np.uint8)) for n in sizes)
    pic = work.pic([b.ptr for b in d_dst], pitches, k.up(work.mvf).ptr, k.up(np.frombuffer(bytes(t_refs), np.uint8)).ptr,
                   k.up(np.frombuffer(bytes(work.slices), np.uint8)).ptr, k.up(lut).ptr)
    af = abi.AffineFrame(pic=pic, cus=k.up(work.aff).ptr, jobs_luma=d_jl.ptr, jobs_chroma=d_jc.ptr, n_cus=len(work.aff), n_jobs=work.n_aff_jobs)
    gf = abi.GpmFrame(pic=pic, cus=k.up(work.gpm).ptr, jobs=d_g.ptr, n_cus=len(work.gpm), n_jobs=work.n_gpm_jobs)
    (a_ptr, _), (g_ptr, _) = k.frame(af), k.frame(gf)
    outs = []
    for halves in (False, True):
        for b, s in zip(d_dst, start):
            dev.vvc355_upload(b.ptr, s.ctypes.data, s.nbytes)
        for b in (d_jl, d_jc, d_g):
            z = np.zeros(b.nbytes, np.uint8)
            dev.vvc355_upload(b.ptr, z.ctypes.data, z.nbytes)
        if halves:
            dev.vvc355_affine_frame_build(None, a_ptr, ctypes.addressof(af))
            dev.vvc355_gpm_frame_build(None, g_ptr, ctypes.addressof(gf))
            dev.vvc355_affine_frame_predict(None, bd, a_ptr, ctypes.addressof(af))
            dev.vvc355_gpm_frame_predict(None, bd, g_ptr, ctypes.addressof(gf))
        else:
            dev.vvc355_affine_frame_pass(None, bd, a_ptr, ctypes.addressof(af))
            dev.vvc355_gpm_frame_pass(None, bd, g_ptr, ctypes.addressof(gf))
        dev.vvc355_stream_sync(None)
        assert dev.vvc355_last_error() == 0
        outs.append([b.to_host(np.uint8, (b.nbytes,)) for b in d_dst + [d_jl, d_jc, d_g]])
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    assert all(o.any() for o in outs[0]) and any(np.any(o != s.view(np.uint8).ravel()) for o, s in zip(outs[0], start))

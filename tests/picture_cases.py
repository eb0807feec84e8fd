"""Cases for vvc355_picture_pass and the pieces that came with it (vvc355_lmcs_frame_pass, vvc355_recon_order_check, the events): the
vvc355_picture of a set of stages, the inverse-LMCS pictures with their numpy expectation and their per-CTB vvc355_lmcs_batch jobs, host
frames with made-up addresses that every stage check accepts (for the validation tests, which launch nothing), the RECON tables whose
ticket orders are checked, and the end-to-end pictures put together from ref_pass_cases, ciip_frame_cases, ts_tb_cases and
inter_frame_cases.  Those modules are imported, never changed.  Used by tests/test_picture_cpu.py, tests/test_picture_gpu.py and
tools/picture_pass_time.py."""
import ctypes
from types import SimpleNamespace

import numpy as np

import recon_cases
from ffvvc_amd import abi, batch

SEED = 0x5EED71C0


# ---------------------------------------------------------------------------------------------------------------- the picture descriptor

def picture(stages=(), alf_work=0, recon_tables=None, refs=(), done=0):
    """abi.Picture of `stages` = {stage name: (device address, host ctypes frame)}.  recon_tables = (ctus, order) host numpy arrays for the
    order check.  The frames (and the tables) must outlive the call: they are kept on the returned object."""
    p = abi.Picture()
    p.keep = []
    for name, (dev_ptr, frame) in dict(stages).items():
        assert name in abi.PIC_STAGES, name
        ref = getattr(p, name)
        ref.dev, ref.host = dev_ptr or 0, ctypes.addressof(frame) if frame is not None else 0
        p.keep.append(frame)
    p.alf_work = alf_work
    if recon_tables is not None:
        ctus, order = (np.ascontiguousarray(a) for a in recon_tables)
        p.recon_ctus_host, p.recon_order_host = ctus.ctypes.data, order.ctypes.data
        p.keep += [ctus, order]
    for i, ev in enumerate(refs):
        p.refs[i] = ev or 0
    p.n_refs, p.done = len(refs), done or 0
    return p


def run(dev, stream, bd, pic):
    return dev.vvc355_picture_pass(stream, bd, ctypes.addressof(pic))


def decode(ret):
    return abi.pic_stage(ret), abi.pic_code(ret)


# ---------------------------------------------------------------------------------------------------------------- inverse LMCS pictures

# bit depth, width, height, CTB log2, row pitch in BYTES (None: 256-byte multiple)
LMCS_CASES = [
    dict(bd=8, width=100, height=52, ctb_log2=5, pitch=None),          # right CTB 4 samples wide, bottom CTB 20 rows
    dict(bd=10, width=136, height=72, ctb_log2=6, pitch=None),
    dict(bd=12, width=264, height=136, ctb_log2=7, pitch=None),         # right CTB 8 wide
    dict(bd=8, width=100, height=52, ctb_log2=5, pitch=101),           # unaligned rows: the per-sample path
]
LMCS_FILL = 0xC3                    # the byte of the pitch padding
_lmcs = {}


def lmcs_case(i):
    """Three slices with sh_lmcs_used_flag 1 / 0 / 1 and one CTB that belongs to no slice (slice_idx -1).  Made once; nobody writes to it."""
    if i not in _lmcs:
        c = LMCS_CASES[i]
        rng = np.random.default_rng(SEED + i)
        bd, w, h, log2 = c["bd"], c["width"], c["height"], c["ctb_log2"]
        dt = np.uint8 if bd == 8 else np.uint16
        cw, ch = (w + (1 << log2) - 1) >> log2, (h + (1 << log2) - 1) >> log2
        n = cw * ch
        assert n >= 4
        slice_idx = np.minimum(np.arange(n) * 3 // n, 2).astype(np.int16)
        hole = n // 2 + (1 if n > 4 else 0)
        slice_idx[hole] = -1
        assert set(slice_idx.tolist()) == {-1, 0, 1, 2}
        plane = rng.integers(0, 1 << bd, size=(h, w), dtype=np.int64).astype(dt)
        lut = rng.integers(0, 1 << bd, size=1 << bd, dtype=np.int64).astype(dt)        # fc->ps.lmcs.inv_lut: any table does
        pitch = c["pitch"] or batch.plane_pitch(w, plane.itemsize)
        assert pitch >= w * plane.itemsize
        _lmcs[i] = SimpleNamespace(bd=bd, width=w, height=h, ctb_log2=log2, cw=cw, ch=ch, pitch=pitch, plane=plane, lut=lut, slice_idx=slice_idx,
                                   used=np.array([1, 0, 1], np.uint8), n_slices=3, isz=plane.itemsize)
    return _lmcs[i]


def lmcs_bytes(c, plane):
    """The device image of a plane: rows at c.pitch bytes, the padding filled with LMCS_FILL."""
    out = np.full((c.height, c.pitch), LMCS_FILL, np.uint8)
    out[:, :c.width * c.isz] = np.ascontiguousarray(plane).view(np.uint8).reshape(c.height, -1)
    return out


def lmcs_mask(width, height, ctb_log2, slice_idx, used):
    """Samples (height x width, bool) of the CTBs whose slice uses LMCS; slice indices outside the flags' range are holes."""
    cw = (width + (1 << ctb_log2) - 1) >> ctb_log2
    ys, xs = np.arange(height)[:, None] >> ctb_log2, np.arange(width)[None, :] >> ctb_log2
    s = np.asarray(slice_idx)[ys * cw + xs].astype(np.int64)
    ok = (s >= 0) & (s < len(used))
    return ok & (np.asarray(used)[np.clip(s, 0, len(used) - 1)] != 0)


def lmcs_expected(c, plane=None):
    """lmcs.filter by numpy (vvc_filter_template.c:25: dst[x] = lut[dst[x]]) on the CTBs of slices that use LMCS."""
    plane = c.plane if plane is None else plane
    return np.where(lmcs_mask(c.width, c.height, c.ctb_log2, c.slice_idx, c.used), c.lut[plane], plane).astype(plane.dtype)


def lmcs_frame(c, plane_ptr, lut_ptr, slice_ptr, used_ptr, pitch=None):
    f = abi.LmcsFrame()
    f.plane, f.inv_lut, f.slice_idx, f.slice_lmcs_used = plane_ptr, lut_ptr, slice_ptr, used_ptr
    f.stride, f.width, f.height, f.ctb_width, f.ctb_height = pitch or c.pitch, c.width, c.height, c.cw, c.ch
    f.n_slices, f.ctb_log2 = c.n_slices, c.ctb_log2
    return f


def lmcs_jobs(c, plane_ptr, lut_ptr, pitch=None):
    """What a host builds for vvc355_lmcs_batch today: one vvc355_blend_job per CTB of a slice that uses LMCS."""
    pitch = pitch or c.pitch
    ctb = 1 << c.ctb_log2
    jobs = []
    for rs in range(c.cw * c.ch):
        s = int(c.slice_idx[rs])
        if not (0 <= s < c.n_slices) or not c.used[s]:
            continue
        x0, y0 = (rs % c.cw) * ctb, (rs // c.cw) * ctb
        jobs.append((plane_ptr + y0 * pitch + x0 * c.isz, min(ctb, c.width - x0), min(ctb, c.height - y0)))
    arr = batch.job_array(abi.BlendJob, len(jobs))
    for j, (dst, w, h) in zip(arr, jobs):
        j["dst"], j["src0"], j["dst_stride"], j["w"], j["h"] = dst, lut_ptr, pitch, w, h
    return arr


# ---------------------------------------------------------------------------------------------------------------- frames the checks accept

def valid_frames(bd=10):
    """Host frames with made-up device addresses that pass every stage's own check, for pictures that must be refused (nothing is launched):
    {stage: frame}.  The record counts are positive, so that a picture which got past validation by mistake would launch."""
    A = iter(range(0x10000, 0x1000000, 0x1000))
    nxt = lambda: next(A)          # noqa: E731
    width, height, log2 = 328, 200, 6
    cw, ch = 6, 4
    f = {}
    ci = abi.CiipFrame()
    p = ci.pic
    p.dst[0], p.dst[1], p.dst[2], p.mvf, p.refs, p.slices = (nxt() for _ in range(6))
    p.dst_stride[0], p.dst_stride[1], p.dst_stride[2], p.mvf_stride = 1024, 512, 512, 82
    p.width, p.height, p.hs, p.vs, p.chroma_format_idc, p.pixel_shift = width, height, 1, 1, 1, int(bd > 8)
    ci.cus, ci.jobs, ci.scratch, ci.slice_idx, ci.ctb_to_col_bd, ci.ctb_to_row_bd = (nxt() for _ in range(6))       # cmds = 0: prediction only
    ci.n_cus, ci.n_jobs, ci.scratch_len, ci.n_slices, ci.n_cmds, ci.ctb_width, ci.ctb_height, ci.ctb_log2 = 10, 60, 4096, 2, 40, cw, ch, log2
    f["ciip"] = ci
    it = abi.IntraTbFrame()
    it.tus, it.coeffs, it.n_tus, it.range, it.bd = nxt(), nxt(), 5, 15, bd
    for k in range(6):
        it.class_first[k] = k
    f["intra_tb"] = it
    for name, ty, nb in (("inter_tb", abi.InterTbFrame, abi.INTER_TB_BINS), ("ts_tb", abi.TsTbFrame, abi.TS_TB_CLASSES)):
        t = ty()
        t.tus, t.coeffs, t.plane[0], t.plane[1], t.plane[2] = (nxt() for _ in range(5))
        t.stride[0], t.stride[1], t.stride[2], t.width, t.height = 1024, 512, 512, width, height
        t.n_tus, t.hs, t.vs, t.size_y, t.range, t.bd = 2 * nb, 1, 1, 64, 15, bd
        first = t.bin_first if name == "inter_tb" else t.class_first
        for chn in range(2):
            for k in range(nb + 1):
                first[chn][k] = chn * nb + k
        f[name] = t
    b = abi.BsRecFrame()
    b.cu, b.tu, b.ctu_first_cu, b.ctu_first_tu, b.mvf, b.ref_poc, b.slice_idx, b.ctb_to_col_bd, b.ctb_to_row_bd = (nxt() for _ in range(9))
    for d in range(2):
        for c in range(3):
            b.bs[d][c] = nxt()
        b.max_len_p[d], b.max_len_q[d] = nxt(), nxt()
    b.n_cu, b.n_tu, b.unit_pitch, b.mvf_pitch = 30, 60, 82, 82
    b.width, b.height, b.ctb_width, b.ctb_height, b.ctb_log2, b.hs, b.vs, b.n_comp = width, height, cw, ch, log2, 1, 1, 3
    f["bs_rec"] = b
    q = abi.QpRecFrame()
    q.cu, q.tu, q.ctu_first_cu, q.ctu_first_tu, q.cu_qp, q.tu_qp_c, q.qp_y, q.qp_c[0], q.qp_c[1] = (nxt() for _ in range(9))
    q.n_cu, q.n_tu, q.unit_pitch, q.width, q.height, q.ctb_width, q.ctb_height, q.ctb_log2, q.n_comp = 30, 60, 82, width, height, cw, ch, log2, 3
    f["qp_rec"] = q
    m = abi.LmcsFrame()
    m.plane, m.inv_lut, m.slice_idx, m.slice_lmcs_used = (nxt() for _ in range(4))
    m.stride, m.width, m.height, m.ctb_width, m.ctb_height, m.n_slices, m.ctb_log2 = 1024, width, height, cw, ch, 2, log2
    f["lmcs"] = m
    return f


# one way to break each checked stage, and the code its own entry returns for it: (stage, field path, value, code name)
MALFORMED = [
    ("ciip", "ctb_log2", 4, "CIIP_E_CTB"),
    ("intra_tb", "range", 21, "INTRA_TB_E_RANGE"),
    ("bs_rec", "unit_pitch", 81, "BS_REC_E_PITCH"),
    ("qp_rec", "cu_qp", 0, "QP_REC_E_SIDECAR"),
    ("inter_tb", "hs", 2, "INTER_TB_E_SHIFT"),
    ("ts_tb", "levels", 0x7000, "TS_TB_E_LEVELS"),
    ("lmcs", "stride", 327 * 2, "LMCS_FRAME_E_STRIDE"),
]
STAGE_ID = {n: getattr(abi, "PIC_STAGE_" + n.upper()) for n in abi.PIC_STAGES}
# error codes of the TB passes are not named in abi.py: as the header numbers them
CODES = dict(INTRA_TB_E_RANGE=-3, INTER_TB_E_SHIFT=-6, TS_TB_E_LEVELS=-4)


def code_of(name):
    return CODES[name] if name in CODES else getattr(abi, name)


# ---------------------------------------------------------------------------------------------------------------- RECON tables and orders

def recon_tables():
    """(name, ctus, ncx, ncy) of the pictures whose ticket orders are checked: the RECON case lists (all intra, mixed with CIIP, whole
    inter CTUs, LIGHT CTUs that wait for the luma of their left / upper neighbour, the end-to-end picture of ciip_frame_cases)."""
    out = []
    rng = np.random.default_rng(SEED + 100)
    for name, (w, h, log2, kw) in {
        "all intra": (456, 264, 6, dict(intra_frac=1.0, n_slices=3, tiles=True)),
        "mixed with CIIP": (712, 456, 7, dict(intra_frac=0.5, ciip_frac=0.3)),
        "whole inter CTUs": (712, 456, 6, dict(intra_ctu=np.random.default_rng(SEED + 101).random(12 * 8) < 0.4)),
    }.items():
        work = recon_cases.ReconWork(rng, w, h, log2, 1, 1, **kw)
        out.append((name, work.ctus, work.ncx, work.ncy))
    w, h, log2 = 640, 384, 6
    n = (w >> log2) * (h >> log2)
    intra = np.random.default_rng(SEED + 102).random(n) < 0.35
    work = recon_cases.ReconWork(rng, w, h, log2, 1, 1, intra_ctu=intra, lmcs=True, resid_ctu=~intra, split=(0.7, 0.2))
    flags = work.ctus["flags"]
    assert (flags & abi.RECON_CTU_LIGHT).any() and (flags & abi.RECON_CTU_LUMA_LEFT).any() and (flags & abi.RECON_CTU_LUMA_UP).any()
    out.append(("LIGHT CTUs", work.ctus, work.ncx, work.ncy))
    import ciip_frame_cases as cc
    work, _p = cc.e2e_work()
    out.append(("CIIP end to end", work.ctus, work.ncx, work.ncy))
    return out


def waits_for(ctus, ncx, rs):
    """The CTUs `rs` waits for, as include/vvc_mi355.h states the rule of vvc355_recon_ctu.flags."""
    ry, rx = divmod(int(rs), ncx)
    fl = int(ctus[rs]["flags"])
    if fl & abi.RECON_CTU_LIGHT:
        cand = [rs - 1 if (fl & abi.RECON_CTU_LUMA_LEFT) and rx else -1, rs - ncx if (fl & abi.RECON_CTU_LUMA_UP) and ry else -1]
    else:
        cand = [rs - 1 if rx else -1, rs - ncx - 1 if rx and ry else -1, rs - ncx if ry else -1, rs - ncx + 1 if ry and rx + 1 < ncx else -1]
    return [d for d in cand if d >= 0 and ctus[d]["n_cmd"]]


def order_check(lib, ctus, ncx, ncy, order):
    order = np.ascontiguousarray(order, np.int32)
    table = np.ascontiguousarray(ctus)
    return lib.vvc355_recon_order_check(table.ctypes.data, ncx, ncy, order.ctypes.data if len(order) else None, len(order))


# ---------------------------------------------------------------------------------------------------------------- device plumbing

class Keep:
    """Uploads that stay alive until the test ends."""

    def __init__(self):
        self.keep = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        self.keep.append(batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a))
        return self.keep[-1]

    def frame(self, f):
        """(device address, the host frame): a stage of picture()."""
        self.keep.append(f)
        return self.up(np.frombuffer(bytes(f), np.uint8)).ptr, f


class ReconPicture:
    """The end-to-end picture of ciip_frame_cases.e2e_work() on the device — CIIP build + predict, RECON with the host order tables, inverse
    LMCS on the CTBs of slice 0 — and what the oracle makes of it: orc_bipred_block on the expected jobs, orc_recon_frame_pass, then the
    numpy LUT.  stages() are the picture's stages; reset() restores planes, commands and scratch for another run."""

    def __init__(self, dev, orc, order="critical"):
        import bipred_cases as bc
        import ciip_frame_cases as cc
        from conftest import P
        orc.orc_recon_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.ReconFrame)]
        orc.orc_recon_frame_pass.restype = None
        self.dev, k = dev, Keep()
        self.k = k
        work, p = cc.e2e_work()
        self.work, self.p = work, p
        bd, isz = p.bd, p.isz
        self.bd = bd
        rng = np.random.default_rng(0xC11BE2E)
        dims, refs, lut = cc.pictures(rng, p, bd)
        self.dims = dims
        planes = [bc.smooth_picture(rng, ph, pw, bd, scale=16) for (pw, ph) in dims]
        resid = rng.integers(-(1 << (bd - 3)), 1 << (bd - 3), size=max(1, work.resid_len)).astype(np.int32)
        model = recon_cases.ReconWork.lmcs_model(np.random.default_rng(0x1A5C + bd), bd)
        is_ciip = work.cmds["kind"] == abi.RECON_CIIP
        weights = cc.unit_weights(p)
        self.raster = work.order.copy()
        self.order = recon_cases.critical_order(dev, work.ctus, work.ncx, work.ncy) if order == "critical" else self.raster
        self.inv_lut = np.random.default_rng(SEED + 200).integers(0, 1 << bd, size=1 << bd, dtype=np.int64).astype(planes[0].dtype)
        self.used = np.array([1, 0], np.uint8)

        # ---- oracle
        scratch = np.zeros(p.scratch_len, planes[0].dtype)
        want = [pl.copy() for pl in planes]
        h_jobs = cc.expect_jobs(p, lambda c: (want[c].ctypes.data, dims[c][0] * isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * isz),
                                scratch.ctypes.data, lut.ctypes.data)
        cc.call(orc.orc_bipred_block, bd, h_jobs)
        hc = work.bind(resid.ctypes.data, scratch.ctypes.data, isz)
        for u, cu in enumerate(p.cus):
            hc["joint"][cu["cmd"]] = weights[u]
        hf = work.frame([P(pl) for pl in want], [d[0] * isz for d in dims], hc.ctypes.data, work.ctus.ctypes.data, self.raster.ctypes.data, 0,
                        work.slice_idx.ctypes.data, work.col_bd.ctypes.data, work.row_bd.ctypes.data, lmcs_ptr=ctypes.addressof(model))
        orc.orc_recon_frame_pass(bd, ctypes.byref(hf))
        self.recon = want
        mask = lmcs_mask(p.width, p.height, p.ctb_log2, work.slice_idx, self.used)
        assert mask.any() and not mask.all()
        self.want = [np.where(mask, self.inv_lut[want[0]], want[0]).astype(want[0].dtype), want[1], want[2]]
        self.start = planes

        # ---- device
        self.pitched = [batch.to_pitched(pl) for pl in planes]
        self.d_planes = [k.up(pl) for pl in self.pitched]
        self.pitches = pitches = [pl.shape[1] * isz for pl in self.pitched]
        d_res = k.up(resid)
        dcmd = work.bind(d_res.ptr, 0, isz)
        dcmd["resid"][is_ciip] = 0
        dcmd["joint"][is_ciip] = 0
        self.cmds0 = dcmd.view(np.uint8).copy()
        self.d_cmds, d_ctus, d_order = k.up(self.cmds0), k.up(work.ctus), k.up(self.order)
        d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(work.ncx * work.ncy))
        k.keep.append(d_state)
        d_slice, d_col, d_row = (k.up(a) for a in (work.slice_idx, work.col_bd, work.row_bd))
        d_model = k.up(np.frombuffer(bytes(model), np.uint8))
        d_ref = [[[k.up(batch.to_pitched(refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
        d_reft = k.up(np.frombuffer(bytes(cc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], pitches)), np.uint8))
        self.d_mvf = d_mvf = k.up(p.mvf)
        d_sl, d_lut, d_cus = k.up(np.frombuffer(bytes(p.slices), np.uint8)), k.up(lut), k.up(p.cus)
        d_jobs = batch.DeviceBuffer(p.n_jobs * cc.BIPRED_JOB_DT.itemsize)
        k.keep.append(d_jobs)
        self.scratch0 = np.zeros(p.scratch_len, planes[0].dtype)
        self.d_scratch = k.up(self.scratch0)
        self.cf = p.frame(p.pic([b.ptr for b in self.d_planes], pitches, d_mvf.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr), d_cus.ptr, d_jobs.ptr,
                          self.d_scratch.ptr, self.d_cmds.ptr, d_slice.ptr, d_col.ptr, d_row.ptr)
        self.rf = work.frame([b.ptr for b in self.d_planes], pitches, self.d_cmds.ptr, d_ctus.ptr, d_order.ptr, d_state.ptr, d_slice.ptr, d_col.ptr,
                             d_row.ptr, lmcs_ptr=d_model.ptr)
        c = SimpleNamespace(width=p.width, height=p.height, cw=work.ncx, ch=work.ncy, n_slices=2, ctb_log2=p.ctb_log2, pitch=pitches[0])
        self.lf = lmcs_frame(c, self.d_planes[0].ptr, k.up(self.inv_lut).ptr, d_slice.ptr, k.up(self.used).ptr)
        self._stages = dict(ciip=k.frame(self.cf), recon=k.frame(self.rf), lmcs=k.frame(self.lf))

    def stages(self):
        return dict(self._stages)

    def tables(self):
        return self.work.ctus, self.order

    def reset(self):
        for b, pl in zip(self.d_planes, self.pitched):
            self.dev.vvc355_upload(b.ptr, pl.ctypes.data, pl.nbytes)
        self.dev.vvc355_upload(self.d_cmds.ptr, self.cmds0.ctypes.data, self.cmds0.nbytes)
        self.dev.vvc355_upload(self.d_scratch.ptr, self.scratch0.ctypes.data, self.scratch0.nbytes)

    def planes(self):
        return [b.to_host(pl.dtype, pl.shape)[:, :d[0]] for b, pl, d in zip(self.d_planes, self.pitched, self.dims)]


# ---------------------------------------------------------------------------------------------------------------- one picture, both halves

def unit_tables(work, p, rng):
    """A bs_cases.BsTables of the reconstruction picture: its coding units are the picture's own (the rectangles the RECON commands name;
    a CTU the walk does not visit is one unit), its MvField table is the picture's (p.mvf: what the CIIP builder reads), so the motion
    records reproduce that table; one luma transform unit and one chroma transform unit per coding unit, coded flags drawn.  Slices and
    tiles are the picture's."""
    import bs_cases

    units = {}
    for k in work.cmds:
        x, y, w, h = (int(k[n]) for n in ("cu_x0", "cu_y0", "cb_width", "cb_height"))
        if w and h:
            units.setdefault((y >> work.ctb_log2) * work.ncx + (x >> work.ctb_log2), set()).add((x, y, w, h))
    src = np.ascontiguousarray(p.mvf).view(np.dtype(abi.MvField)).reshape(p.mvf.shape).copy()
    src["ref_idx"] = np.maximum(src["ref_idx"], 0)               # the unused list's index is never read; the tables keep it in range

    class UnitTables(bs_cases.BsTables):
        def _ctb(self, _rng, x0, y0, ctb, gmv, inter_frac):
            rs = (y0 >> self.ctb_log2) * self.cw + (x0 >> self.ctb_log2)
            leaves = sorted(units.get(rs, {(x0, y0, min(ctb, self.width - x0), min(ctb, self.height - y0))}), key=lambda u: (u[1], u[0]))
            covered = np.zeros((ctb // 4, ctb // 4), np.int32)
            for (x, y, w, h) in leaves:
                s = np.s_[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
                covered[(y - y0) // 4:(y - y0 + h) // 4, (x - x0) // 4:(x - x0 + w) // 4] += 1
                self.cbx[s], self.cby[s], self.cbw[s], self.cbh[s] = x, y, w, h
                self.mvf[s] = src[s]
                self.cu_recs.append((x, y, w, h, 0, 0))
                flat = src[s].reshape(-1)
                if all(flat[i].tobytes() == flat[0].tobytes() for i in range(len(flat))):
                    self.mv_recs.append((x, y, w, h, flat[0].tobytes()))
                else:                                             # the background motion of the picture changes every 8x8
                    for by in range(0, h, 4):
                        for bx in range(0, w, 4):
                            self.mv_recs.append((x + bx, y + by, 4, 4, src[(y + by) // 4, (x + bx) // 4].tobytes()))
                ts = self._fill_tu(0, x, y, w, h, 0)
                self.cbf0[ts] = int(rng.random() < self.cbf_p)
                self.tu_recs.append((x, y, w, h, int(self.cbf0[y // 4, x // 4]), 0))
                ts = self._fill_tu(1, x, y, w, h, 1)
                self.cbf1[ts], self.cbf2[ts], self.joint[ts] = int(rng.random() < 0.3), int(rng.random() < 0.3), int(rng.random() < 0.1)
                self._tu1_rec(x, y, w, h)
            assert np.all(covered[:min(ctb, self.height - y0) // 4, :min(ctb, self.width - x0) // 4] == 1), "the units do not tile the CTU"

    t = UnitTables(rng, work.width, work.height, work.ctb_log2, n_slices=int(work.slice_idx.max()) + 1, tiles=False, lfase=0, lfate=0, hs=work.hs, vs=work.vs)
    t.slice_idx, t.col_bd, t.row_bd = work.slice_idx, work.col_bd, work.row_bd
    assert t.mvf.tobytes() == src.tobytes()
    return t


def whole_picture(rp):
    """The filter half that goes with a ReconPicture: (deblocking picture, SAO / ALF picture) as ref_pass_cases makes them, on tables and
    records derived from the reconstruction picture's units, with drawn QPs, deblocking offsets and per-CTB SAO / ALF parameters."""
    import qp_rec_cases as qc
    import ref_pass_cases as pc
    import bs_rec_cases as rc
    rng = np.random.default_rng(SEED + 500)
    t = unit_tables(rp.work, rp.p, rng)
    bd, qp_bd = rp.bd, 6 * (rp.bd - 8)
    (cu, cu_first), (tu, tu_first), _ = rc.grouped(t)
    rec = qc.Pic(g=t, cu=cu, tu=tu, cu_first=cu_first, tu_first=tu_first, cu_qp=rng.integers(-qp_bd, 64, size=len(cu)).astype(np.int8),
                 tu_qp_c=rng.integers(0, 64 + qp_bd, size=(len(tu), 2)).astype(np.int8))
    dbp = (2 * rng.integers(-12, 13, size=(t.cw * t.ch, 6))).astype(np.int8)
    dp = pc._finish_deblock("P0", bd, 3, t, rp.want, qc.expected(rec), dbp, None, rec)
    fp = pc.draw_filter("P0", rng, bd, (1, 1), 3, t.ctb_log2, None, dp.n_slices, True, (0, 0), t=t, planes=False)
    return dp, fp

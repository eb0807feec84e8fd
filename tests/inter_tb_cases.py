"""Transform blocks of the coding units outside the in-order pass for vvc355_inter_tb_pass: block specs on a small picture, their 16-byte
records grouped by channel type and shape bin, the oracle walk (luma blocks, then every 64x64 unit's chroma scale from the reconstructed
luma, then chroma blocks: orc_dequant -> orc_derive_transform_type -> orc_itx -> add / scaled add / joint add) and the device runs — the
new entry, and the path it replaces (vvc355_itx_frame_build -> vvc355_itx_shape_batch_lv per shape -> vvc355_lmcs_vpdu_scale_pass ->
vvc355_lmcs_chroma_resid_batch).

A spec is a dict: c_idx, x0, y0 (the component's samples), lw, lh, c (int32 levels, shape (h, w)), nzw, nzh, qp, dep, tu_flags, mts_idx,
joint (bits 0-3 of vvc355_recon_cmd.joint), keep, cu (luma origin of the block's coding unit; None = the block's own position).  Optional,
for records that break the contract: bin / ch (where the record is filed), flags_or / joint_mts_or (bits ORed into the record), off_add
(added to coeff_off), rec_lw (the record's log2_w), bad (the walk leaves the block out)."""
import ctypes

import numpy as np

import levels_cases as lc
from ffvvc_amd import abi, batch

SENT = 0x7EADBEEF
GAP = 64                                   # sentinel words in front of, between and behind the blocks' arena slots
NB = abi.INTER_TB_BINS


def shape_bin(lw, lh):
    return (lw - 2) * 5 + (lh - 2) if lw >= 2 and lh >= 2 else 25


def spec(c_idx, x0, y0, lw, lh, c, nzw, nzh, qp=30, dep=0, tu_flags=0, mts_idx=0, joint=0, keep=False, cu=None, **raw):
    s = dict(c_idx=c_idx, x0=x0, y0=y0, lw=lw, lh=lh, c=c, nzw=nzw, nzh=nzh, qp=qp, dep=dep, tu_flags=tu_flags, mts_idx=mts_idx, joint=joint,
             keep=keep, cu=cu)
    s.update(raw)
    return s


def random_spec(rng, c_idx, x0, y0, lw, lh, max_nz=16, **kw):
    w, h = 1 << lw, 1 << lh
    nzw, nzh = int(rng.integers(1, min(w, max_nz) + 1)), int(rng.integers(1, min(h, max_nz) + 1))
    kw.setdefault("qp", int(rng.integers(0, 52)))
    kw.setdefault("dep", int(rng.integers(0, 2)))
    return spec(c_idx, x0, y0, lw, lh, lc.windowed_block(rng, w, h, nzw, nzh), nzw, nzh, **kw)


class Picture:
    """Three planes of prediction samples, the chroma format, the unit size of the chroma scale and (optionally) an LMCS model."""

    def __init__(self, planes, bd, hs=1, vs=1, size_y=64, ctb_log2=7, model=None):
        self.planes, self.bd, self.hs, self.vs, self.size_y, self.ctb_log2, self.model = planes, bd, hs, vs, size_y, ctb_log2, model
        self.height, self.width = planes[0].shape
        self.isz = planes[0].itemsize
        assert planes[1].shape == planes[2].shape == (self.height >> vs, self.width >> hs)
        self.ls = int(size_y).bit_length() - 1
        self.ux, self.uy = (self.width + size_y - 1) // size_y, (self.height + size_y - 1) // size_y

    @classmethod
    def random(cls, rng, bd, width, height, hs=1, vs=1, lmcs=False, **kw):
        dt = np.uint8 if bd == 8 else np.uint16
        dims = [(height, width), (height >> vs, width >> hs), (height >> vs, width >> hs)]
        planes = [rng.integers(0, 1 << bd, size=d, dtype=np.int64).astype(dt) for d in dims]
        model = None
        if lmcs:
            import recon_cases
            model = recon_cases.ReconWork.lmcs_model(rng, bd)
        return cls(planes, bd, hs, vs, model=model, **kw)

    def luma_pos(self, s):
        return (s["x0"] << (self.hs if s["c_idx"] else 0), s["y0"] << (self.vs if s["c_idx"] else 0))

    def unit_of(self, s, rule="cu"):
        """(unit column, unit row) whose scale the block takes: of its coding unit's origin (the reference's rule), or of the block itself."""
        x, y = self.luma_pos(s) if (rule == "block" or s["cu"] is None) else s["cu"]
        return x >> self.ls, y >> self.ls


def bind_oracle(orc):
    orc.orc_derive_transform_type.restype = ctypes.c_int
    orc.orc_derive_transform_type.argtypes = [ctypes.c_int] * 6
    orc.orc_lmcs_chroma_resid_block.argtypes = [ctypes.c_int, ctypes.POINTER(abi.LmcsResidJob), ctypes.POINTER(abi.LmcsModel)]
    orc.orc_lmcs_chroma_resid_block.restype = None
    orc.orc_lmcs_vpdu_scale_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.LmcsScaleFrame)]
    orc.orc_lmcs_vpdu_scale_pass.restype = None
    orc.orc_lmcs_chroma_scale_flat.argtypes = [ctypes.c_int, ctypes.POINTER(abi.LmcsScaleJob)]
    orc.orc_lmcs_chroma_scale_flat.restype = ctypes.c_int


def tr_type(orc, s):
    return orc.orc_derive_transform_type(s["tu_flags"], s["mts_idx"], 0, s["c_idx"], 1 << s["lw"], 1 << s["lh"])


def oracle_residual(orc, s, bd, rbits=15):
    co = np.ascontiguousarray(s["c"], np.int32).copy()
    orc.orc_dequant(co.ctypes.data, s["lw"], s["lh"], 0, 0, s["nzw"] - 1, s["nzh"] - 1, s["qp"], 0, s["dep"], bd, rbits, None, 1, -1)
    t = tr_type(orc, s)
    assert orc.orc_itx(t & 15, t >> 4, s["lw"], s["lh"], co.ctypes.data, s["nzw"], s["nzh"], rbits, bd) == 0, (s["lw"], s["lh"], t)
    return co


def unit_maps(pic):
    """One slice, one tile: the maps vvc355_lmcs_vpdu_scale_pass reads for neighbour availability."""
    ctb = 1 << pic.ctb_log2
    ncx, ncy = (pic.width + ctb - 1) // ctb, (pic.height + ctb - 1) // ctb
    return ncx, np.zeros(ncx * ncy, np.int16), np.zeros(ncx + 1, np.int16), np.zeros(ncy + 1, np.int16)


def oracle_scale_table(orc, pic, luma):
    """Every unit's chroma scale from a luma plane (lmcs_derive_chroma_scale per unit)."""
    ncx, sl, col, row = unit_maps(pic)
    out = np.zeros(pic.ux * pic.uy, np.int16)
    luma = np.ascontiguousarray(luma)
    f = abi.LmcsScaleFrame()
    f.luma, f.scale, f.model, f.luma_stride = luma.ctypes.data, out.ctypes.data, ctypes.addressof(pic.model), pic.width * pic.isz
    f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = sl.ctypes.data, col.ctypes.data, row.ctypes.data
    f.width, f.height, f.ctb_width, f.ctb_log2, f.size_y = pic.width, pic.height, ncx, pic.ctb_log2, pic.size_y
    orc.orc_lmcs_vpdu_scale_pass(pic.bd, ctypes.byref(f))
    return out


def oracle_unit_scale(orc, pic, luma, ux, uy):
    """orc_lmcs_chroma_scale_flat of one unit (one slice, one tile: a neighbour exists wherever the picture has one)."""
    luma = np.ascontiguousarray(luma)
    j = abi.LmcsScaleJob()
    j.luma, j.luma_stride = luma.ctypes.data, pic.width * pic.isz
    j.x_vpdu, j.y_vpdu, j.pic_w, j.pic_h, j.size_y = ux * pic.size_y, uy * pic.size_y, pic.width, pic.height, pic.size_y
    j.avail_l, j.avail_t = int(ux > 0), int(uy > 0)
    j.min_bin_idx, j.max_bin_idx = pic.model.min_bin_idx, pic.model.max_bin_idx
    for i in range(17):
        j.pivot[i] = pic.model.pivot[i]
    for i in range(16):
        j.chroma_scale_coeff[i] = pic.model.chroma_scale_coeff[i]
    return orc.orc_lmcs_chroma_scale_flat(pic.bd, ctypes.byref(j))


def oracle_walk(orc, pic, specs, offs, arena0, rule="cu", rbits=15):
    """What the stage leaves: (planes, arena, scale table or None).  Luma blocks first, then the table from the reconstructed luma, then
    chroma.  Specs marked bad are left out.  rule: which unit a scaled block takes its scale from (see Picture.unit_of)."""
    bd, isz = pic.bd, pic.isz
    planes = [np.ascontiguousarray(p).copy() for p in pic.planes]
    arena = arena0.copy()
    table = None
    for ch in (0, 1):
        if ch == 1 and pic.model is not None:
            table = oracle_scale_table(orc, pic, planes[0])
        for i, s in enumerate(specs):
            if (s["c_idx"] > 0) != ch or s.get("bad"):
                continue
            res = oracle_residual(orc, s, bd, rbits)
            w, h, c = 1 << s["lw"], 1 << s["lh"], s["c_idx"]
            if s["keep"]:
                arena[offs[i]:offs[i] + w * h] = res.ravel()
                continue
            for (plane, joint) in [(c, s["joint"] & 8)] + ([(3 - c, s["joint"])] if s["joint"] & 1 else []):
                pw = planes[plane].shape[1]
                dst = planes[plane].ctypes.data + (s["y0"] * pw + s["x0"]) * isz
                if joint & 8:
                    ux, uy = pic.unit_of(s, rule)
                    j = abi.LmcsResidJob()
                    j.dst, j.dst_stride, j.resid, j.w, j.h = dst, pw * isz, res.ctypes.data, w, h
                    j.luma, j.joint = table.ctypes.data + (uy * pic.ux + ux) * 2, joint | 16
                    orc.orc_lmcs_chroma_resid_block(bd, ctypes.byref(j), ctypes.byref(pic.model))
                elif joint & 1:
                    orc.orc_add_residual_joint(bd, dst, res.ctypes.data, w, h, pw * isz, -1 if joint & 2 else 1, (joint >> 2) & 1)
                else:
                    orc.orc_add_residual(bd, dst, res.ctypes.data, w, h, pw * isz)
    return planes, arena, table


def group(specs):
    """The specs in record order (luma, then chroma; inside it by the bin they are filed under; stable) and bin_first[2][27]."""
    key = [(int(s.get("ch", s["c_idx"] > 0)), s.get("bin", shape_bin(s["lw"], s["lh"]))) for s in specs]
    order = sorted(range(len(specs)), key=lambda i: key[i])
    counts = np.zeros((2, NB), np.int64)
    for k in key:
        counts[k] += 1
    cum = np.concatenate([[0], np.cumsum(counts.ravel())])
    bin_first = [[int(cum[ch * NB + k]) for k in range(NB + 1)] for ch in range(2)]
    return [specs[i] for i in order], bin_first


def arena_offsets(specs):
    offs, off = [], GAP
    for s in specs:
        offs.append(off)
        off += (1 << (s["lw"] + s["lh"])) + GAP
    return offs, off


def records(pic, specs, offs):
    tus = batch.job_array(abi.InterTu, len(specs))
    for i, s in enumerate(specs):
        t = tus[i]
        t["coeff_off"], t["x0"], t["y0"] = offs[i] + s.get("off_add", 0), s["x0"], s["y0"]
        t["log2_w"], t["log2_h"], t["nzw"], t["nzh"], t["qp"], t["tu_flags"] = s.get("rec_lw", s["lw"]), s["lh"], s["nzw"], s["nzh"], s["qp"], s["tu_flags"]
        (bx, by), (cx, cy) = pic.unit_of(s, "block"), pic.unit_of(s, "cu")
        assert 0 <= bx - cx <= 1 and 0 <= by - cy <= 1
        t["flags"] = (s["c_idx"] | (abi.INTER_TU_DEP_QUANT if s["dep"] else 0) | (abi.INTER_TU_KEEP if s["keep"] else 0) |
                      (abi.INTER_TU_UNIT_DX if bx > cx else 0) | (abi.INTER_TU_UNIT_DY if by > cy else 0) | s.get("flags_or", 0))
        t["joint_mts"] = s["joint"] | (s["mts_idx"] << 4) | s.get("joint_mts_or", 0)
    return tus


def start_arena(specs, offs, n, lv=None):
    """Sentinels everywhere; the levels of the blocks that are not packed (all of them without `lv`) in their slots."""
    arena = np.full(n, SENT, np.int32)
    for i, s in enumerate(specs):
        if lv is None or lv[i]["flags"] & abi.LEVELS_INT32:
            arena[offs[i]:offs[i] + s["c"].size] = s["c"].ravel()
    return arena


FILL = 0x5A                                 # the byte the pitch padding of the device planes is filled with


def pitched(plane):
    h, w = plane.shape
    out = np.full((h, batch.plane_pitch(w, plane.itemsize)), FILL, np.uint8).view(plane.dtype)
    out[:, :w] = plane
    return out


class DevicePicture:
    """The planes in device memory (pitch padding filled with FILL), the scale table and the vvc355_lmcs_scale_frame of the picture."""

    def __init__(self, pic):
        self.pic = pic
        self.host = [pitched(p) for p in pic.planes]
        self.d_planes = [batch.DeviceBuffer.from_host(p) for p in self.host]
        self.strides = [p.shape[1] * pic.isz for p in self.host]
        self.sf = None
        if pic.model is not None:
            ncx, sl, col, row = unit_maps(pic)
            self.table0 = np.full(pic.ux * pic.uy, -1, np.int16)
            self.d_table = batch.DeviceBuffer.from_host(self.table0)
            self.d_model = batch.DeviceBuffer.from_host(np.frombuffer(bytes(pic.model), np.uint8))
            self.d_maps = [batch.DeviceBuffer.from_host(a) for a in (sl, col, row)]
            sf = abi.LmcsScaleFrame()
            sf.luma, sf.scale, sf.model, sf.luma_stride = self.d_planes[0].ptr, self.d_table.ptr, self.d_model.ptr, self.strides[0]
            sf.slice_idx, sf.ctb_to_col_bd, sf.ctb_to_row_bd = (d.ptr for d in self.d_maps)
            sf.width, sf.height, sf.ctb_width, sf.ctb_log2, sf.size_y = pic.width, pic.height, ncx, pic.ctb_log2, pic.size_y
            self.sf, self.d_sf = sf, batch.DeviceBuffer.from_host(np.frombuffer(bytes(sf), np.uint8))

    def reset(self, dev):
        for d, h in zip(self.d_planes, self.host):
            dev.vvc355_upload(d.ptr, h.ctypes.data, h.nbytes)
        if self.sf is not None:
            dev.vvc355_upload(self.d_table.ptr, self.table0.ctypes.data, self.table0.nbytes)

    def scale_pass(self, dev, stream=None):
        dev.vvc355_lmcs_vpdu_scale_pass(stream, self.pic.bd, self.d_sf.ptr, ctypes.addressof(self.sf))

    def pitched_planes(self, dev):
        dev.vvc355_stream_sync(None)
        return [d.to_host(h.dtype, h.shape) for d, h in zip(self.d_planes, self.host)]

    def planes(self, dev):
        return [p[:, :q.shape[1]] for p, q in zip(self.pitched_planes(dev), self.pic.planes)]

    def expected_pitched(self, planes):
        out = [h.copy() for h in self.host]
        for o, p in zip(out, planes):
            o[:, :p.shape[1]] = p
        return out


class Frame:
    """One run of vvc355_inter_tb_pass: records, arena, optional packed levels and the vvc355_inter_tb_frame (host copy + device copy)."""

    def __init__(self, pic, specs, bin_first, offs, arena, rbits=15, packed=None, dpic=None):
        self.pic, self.n, self.arena0 = pic, len(specs), arena
        self.dpic = DevicePicture(pic) if dpic is None else dpic
        self.d_tus = batch.DeviceBuffer.from_host(records(pic, specs, offs).view(np.uint8) if specs else np.zeros(16, np.uint8))
        self.d_arena = batch.DeviceBuffer.from_host(arena)
        f = abi.InterTbFrame()
        f.tus, f.coeffs, f.n_tus = self.d_tus.ptr, self.d_arena.ptr, self.n
        for c in range(3):
            f.plane[c], f.stride[c] = self.dpic.d_planes[c].ptr, self.dpic.strides[c]
        f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = pic.width, pic.height, pic.hs, pic.vs, pic.size_y, rbits, pic.bd
        f.scale_table = self.dpic.d_table.ptr if pic.model is not None else 0
        for ch in range(2):
            for k in range(NB + 1):
                f.bin_first[ch][k] = bin_first[ch][k]
        self.lv = None if packed is None else packed[1]
        if packed is not None:
            levels, lv = packed
            self.d_lv, self.d_levels = batch.DeviceBuffer.from_host(lv.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
            assert self.d_levels.ptr % 32 == 0
            f.lv, f.levels = self.d_lv.ptr, self.d_levels.ptr
        self.f = f
        self.d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))

    def reset(self, dev):
        dev.vvc355_upload(self.d_arena.ptr, self.arena0.ctypes.data, self.arena0.nbytes)
        self.dpic.reset(dev)

    def launch(self, dev, channels, stream=None):
        return dev.vvc355_inter_tb_pass(stream, self.d_f.ptr, ctypes.addressof(self.f), channels)

    def run(self, dev, stream=None):
        """The whole stage: with chroma residual scaling luma, the scale table, chroma; one call otherwise."""
        if self.pic.model is None:
            return self.launch(dev, 3, stream)
        rc = self.launch(dev, 1, stream)
        self.dpic.scale_pass(dev, stream)
        return rc or self.launch(dev, 2, stream)

    def arena(self, dev):
        dev.vvc355_stream_sync(None)
        return self.d_arena.to_host(np.int32, self.arena0.shape)


class OldPath:
    """The path the entry replaces, on the same (grouped) specs: vvc355_itx_tu records with host-derived transform types ->
    vvc355_itx_frame_build (48-byte jobs + 56-byte residual jobs in device scratch) -> vvc355_itx_shape_batch_lv per bin ->
    vvc355_lmcs_vpdu_scale_pass -> vvc355_lmcs_chroma_resid_batch.  It has no joint records, and it takes a scaled block's unit from the
    block's position.  Its records are ordered by shape bin alone (luma and chroma blocks of a shape share a launch, as in bench.py)."""

    def __init__(self, orc, pic, specs, offs, arena, rbits=15, packed=None, dpic=None):
        assert not any(s["joint"] & 1 for s in specs)
        self.pic, self.n, self.arena0 = pic, len(specs), arena
        bins = [shape_bin(s["lw"], s["lh"]) for s in specs]
        perm = sorted(range(len(specs)), key=lambda i: bins[i])
        self.bin_first = [0] + [int(v) for v in np.cumsum(np.bincount(bins, minlength=NB))]
        self.dpic = DevicePicture(pic) if dpic is None else dpic
        if packed is None:
            packed = lc.pack_all([s["c"] for s in specs], force_int32=set(range(len(specs))))
        levels, lv = packed
        lv = lv[perm]
        tus = batch.job_array(abi.ItxTu, self.n)
        for k, i in enumerate(perm):
            s, t = specs[i], tus[k]
            t["coeff_off"], t["x0"], t["y0"], t["log2_w"], t["log2_h"] = offs[i], s["x0"], s["y0"], s["lw"], s["lh"]
            t["nzw"], t["nzh"], t["c_idx"], t["qp"], t["tr"] = s["nzw"], s["nzh"], s["c_idx"], s["qp"], tr_type(orc, s)
            flags = 1 | (s["dep"] << 1) | (4 if s["keep"] else 0)
            if s["joint"] & 8 and not s["keep"]:
                ux, uy = pic.unit_of(s, "block")
                flags |= 4 | 64 | (int(ux > 0) << 4) | (int(uy > 0) << 5)
            t["flags"] = flags
        self.d_tus, self.d_arena = batch.DeviceBuffer.from_host(tus.view(np.uint8)), batch.DeviceBuffer.from_host(arena)
        self.jsz, self.rsz, self.lsz = ctypes.sizeof(abi.ItxJob), ctypes.sizeof(abi.LmcsResidJob), lv.dtype.itemsize
        self.d_jobs, self.d_rjobs = batch.DeviceBuffer(max(1, self.n) * self.jsz), batch.DeviceBuffer(max(1, self.n) * self.rsz)
        self.d_lv, self.d_levels = batch.DeviceBuffer.from_host(lv.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
        f = abi.ItxFrame()
        f.tus, f.jobs, f.coeffs, f.n_tus = self.d_tus.ptr, self.d_jobs.ptr, self.d_arena.ptr, self.n
        for c in range(3):
            f.plane[c], f.stride[c] = self.dpic.d_planes[c].ptr, self.dpic.strides[c]
        f.range, f.bd, f.pixel_shift = rbits, pic.bd, int(pic.isz == 2)
        f.width, f.height, f.hs, f.vs, f.size_y = pic.width, pic.height, pic.hs, pic.vs, pic.size_y
        if pic.model is not None:
            f.resid_jobs, f.scale_table = self.d_rjobs.ptr, self.dpic.d_table.ptr
        self.f, self.d_f = f, batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
        self.scratch_bytes = self.n * (self.jsz + (self.rsz if pic.model is not None else 0))

    def reset(self, dev):
        dev.vvc355_upload(self.d_arena.ptr, self.arena0.ctypes.data, self.arena0.nbytes)
        self.dpic.reset(dev)

    def build(self, dev, stream=None):
        dev.vvc355_itx_frame_build(stream, self.d_f.ptr, ctypes.addressof(self.f))

    def shapes(self, dev, stream=None):
        bd = self.pic.bd
        for k in range(NB):
            first, cnt = self.bin_first[k], self.bin_first[k + 1] - self.bin_first[k]
            if not cnt:
                continue
            jobs, lv = self.d_jobs.ptr + first * self.jsz, self.d_lv.ptr + first * self.lsz
            if k == 25:
                dev.vvc355_itx_batch_lv(stream, bd, jobs, lv, self.d_levels.ptr, cnt, 8)
            else:
                dev.vvc355_itx_shape_batch_lv(stream, bd, jobs, lv, self.d_levels.ptr, cnt, k // 5 + 2, k % 5 + 2)

    def resid(self, dev, stream=None):
        dev.vvc355_lmcs_chroma_resid_batch(stream, self.pic.bd, self.d_rjobs.ptr, self.n, self.dpic.d_model.ptr)

    def run(self, dev, stream=None):
        self.build(dev, stream)
        self.shapes(dev, stream)
        if self.pic.model is not None:
            self.dpic.scale_pass(dev, stream)
            self.resid(dev, stream)
        return 0

    def arena(self, dev):
        dev.vvc355_stream_sync(None)
        return self.d_arena.to_host(np.int32, self.arena0.shape)


def tiled_specs(rng, pic, luma_shapes, chroma_shapes, scaled_frac=1.0, keep_frac=0.0, coded_p=0.8, tu_flags=(0,), mts=(0,)):
    """A small picture's population: the luma plane and the two chroma planes cut into non-overlapping blocks of the given (lw, lh) shapes
    (one shape per column band of 64 samples, cycling), each coded with probability coded_p.  Chroma blocks are scaled with probability
    scaled_frac when the picture has a model and their area is above 4 (itransform's chroma_scale)."""
    out = []
    for c_idx, shapes in ((0, luma_shapes), (1, chroma_shapes), (2, chroma_shapes)):
        ph, pw = pic.planes[c_idx].shape
        k = 0
        for bx in range(0, pw, 64):
            lw, lh = shapes[k % len(shapes)]
            k += 1
            w, h = 1 << lw, 1 << lh
            for y in range(0, ph - h + 1, h):
                for x in range(bx, min(bx + 64, pw) - w + 1, w):
                    if rng.random() >= coded_p:
                        continue
                    joint = 8 if (c_idx and pic.model is not None and w * h > 4 and rng.random() < scaled_frac) else 0
                    out.append(random_spec(rng, c_idx, x, y, lw, lh, tu_flags=int(rng.choice(tu_flags)), mts_idx=int(rng.choice(mts)) if not c_idx else 0,
                                           joint=joint, keep=bool(rng.random() < keep_frac)))
    return out


def unit_dc_luma(rng, bd, width, height, size=64, noise=3):
    """A luma plane with an independent random DC level per size x size unit plus a few levels of noise: neighbouring units then fall into
    different bins of an LMCS model (a flat-random plane averages to the same bin everywhere)."""
    dt = np.uint8 if bd == 8 else np.uint16
    uy, ux = (height + size - 1) // size, (width + size - 1) // size
    dc = rng.integers(noise, (1 << bd) - noise, size=(uy, ux))
    plane = np.kron(dc, np.ones((size, size), np.int64))[:height, :width] + rng.integers(-noise, noise + 1, size=(height, width))
    return np.clip(plane, 0, (1 << bd) - 1).astype(dt)


LARGE_CUS = [(0, 0, 128, 128), (128, 0, 128, 64), (128, 64, 128, 64), (0, 128, 64, 128), (64, 128, 64, 128), (128, 128, 128, 128)]


def large_cu_case(rng, bd):
    """CtbSizeY 128, 256x256 luma at 4:2:0: coding units of 128x128, 128x64 and 64x128 whose 32x32 chroma blocks (one per component and
    64x64 unit the unit covers) lie in four or two units and all take the scale of the unit of the coding unit's origin; a few of them
    joint; small luma blocks on top of a luma plane with its own DC level per unit.  Returns (picture, specs)."""
    import recon_cases
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [unit_dc_luma(rng, bd, 256, 256)] + [rng.integers(0, 1 << bd, size=(128, 128), dtype=np.int64).astype(dt) for _ in range(2)]
    pic = Picture(planes, bd, 1, 1, 64, 7, recon_cases.ReconWork.lmcs_model(rng, bd))
    specs = []
    for y in range(0, 256, 32):
        for x in range(0, 256, 32):
            if rng.random() < 0.5:
                specs.append(random_spec(rng, 0, x + 8, y + 8, 4, 4, tu_flags=abi.TU_MTS_ENABLED, mts_idx=int(rng.integers(0, 5))))
    for (cx, cy, cw, ch) in LARGE_CUS:
        for uy in range(cy, cy + ch, 64):
            for ux in range(cx, cx + cw, 64):
                if rng.random() < 0.25:                  # a joint transform unit: one record, both planes
                    specs.append(random_spec(rng, int(rng.integers(1, 3)), ux // 2, uy // 2, 5, 5, joint=8 | 1 | (int(rng.integers(0, 4)) << 1), cu=(cx, cy)))
                else:
                    for c in (1, 2):
                        specs.append(random_spec(rng, c, ux // 2, uy // 2, 5, 5, joint=8, cu=(cx, cy)))
    return pic, specs


def unit_rule_split(pic, specs, table):
    """Of the scaled blocks outside their coding unit's first unit: (how many, how many of them would get another scale from their own unit)."""
    far = [s for s in specs if s["joint"] & 8 and pic.unit_of(s, "cu") != pic.unit_of(s, "block")]
    t = table.reshape(pic.uy, pic.ux)
    return len(far), sum(1 for s in far if t[pic.unit_of(s, "cu")[::-1]] != t[pic.unit_of(s, "block")[::-1]])

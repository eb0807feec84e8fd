"""Transform-skip blocks (BDPCM included) for vvc355_ts_tb_pass: block specs on a small picture, their 16-byte records grouped by channel type
and area class, the expectation composed from the oracle (levels -> orc_transform_bdpcm when flagged -> orc_dequant with ts = 1 and the flat
matrix -> the tail as inter_tb_cases.oracle_walk does it) and the device run.  Picture, device picture, arena layout and sentinels are those
of inter_tb_cases.

A spec is a dict: ts (True: what tells it from an inter_tb_cases spec), c_idx, x0, y0 (the component's samples), lw, lh, c (int32 levels,
shape (h, w), zero outside the window), nzw, nzh, qp, bdpcm, vert, joint (bits 0-3 of vvc355_recon_cmd.joint), keep, cu (luma origin of the
block's coding unit; None = the block's own position).  Optional, for records that break the contract: cls / ch (where the record is
filed), flags_or / joint_or / pad (bits ORed into the record), off_add (added to coeff_off), rec_lw / rec_lh (the record's log2_w /
log2_h), bad (the walk leaves the block out)."""
import ctypes

import numpy as np

import inter_tb_cases as tc
import levels_cases as lc
from ffvvc_amd import abi, batch

NC = abi.TS_TB_CLASSES
# every shape transform skip is coded for: sides 4..32 as luma, 2..32 as chroma, at least 8 coefficients
LUMA_SHAPES = [(lw, lh) for lw in range(2, 6) for lh in range(2, 6)]
CHROMA_SHAPES = [(lw, lh) for lw in range(1, 6) for lh in range(1, 6) if lw + lh >= 3]


def area_class(lw, lh):
    return max(0, (lw + lh - 3) // 2)


def spec(c_idx, x0, y0, lw, lh, c, nzw, nzh, qp=30, bdpcm=False, vert=False, joint=0, keep=False, cu=None, **raw):
    s = dict(ts=True, c_idx=c_idx, x0=x0, y0=y0, lw=lw, lh=lh, c=c, nzw=nzw, nzh=nzh, qp=qp, bdpcm=bdpcm, vert=vert, joint=joint, keep=keep, cu=cu)
    s.update(raw)
    return s


def random_spec(rng, c_idx, x0, y0, lw, lh, window=None, bits=None, **kw):
    """Random levels in a random window (or `window` = (nzw, nzh)); about a quarter of the 4x4 tiles of a larger window are emptied."""
    w, h = 1 << lw, 1 << lh
    nzw, nzh = window if window else (int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1)))
    c = lc.windowed_block(rng, w, h, nzw, nzh, bits)
    for ty in range(0, nzh, 4):
        for tx in range(0, nzw, 4):
            if (tx or ty) and rng.random() < 0.25:
                c[ty:ty + 4, tx:tx + 4] = 0
    kw.setdefault("qp", int(rng.integers(4, 52)))
    return spec(c_idx, x0, y0, lw, lh, c, nzw, nzh, **kw)


def saturating_levels(w, h, vert, rbits=15):
    """Levels whose clipped running sum along the BDPCM direction leaves the range at both ends: every line runs up with the largest level,
    then down with the smallest, from a start that differs from line to line."""
    hi, lo = (1 << rbits) - 1, -(1 << rbits)
    n, lines = (h, w) if vert else (w, h)
    c = np.zeros((lines, n), np.int32)
    for l in range(lines):
        if n == 2:                                   # two samples reach one end: the lines alternate
            c[l] = hi if l % 2 == 0 else lo
            continue
        up = 1 + (n - 1) // 2 - l % 2
        c[l, :up] = hi
        c[l, up:] = lo
        c[l, 0] = hi - 3 * l if l % 3 else 5 + l
    return np.ascontiguousarray(c.T) if vert else c


def bdpcm(orc, c, vert, rbits=15):
    out = np.ascontiguousarray(c, np.int32).copy()
    orc.orc_transform_bdpcm(out.ctypes.data, out.shape[1], out.shape[0], int(vert), rbits)
    return out


def oracle_residual(orc, s, bd, rbits=15):
    """The block's residual: transform_bdpcm on the levels, then the scaling process with ts = 1 over the whole block."""
    co = np.ascontiguousarray(s["c"], np.int32).copy()
    w, h = 1 << s["lw"], 1 << s["lh"]
    assert co.shape == (h, w) and not co[s["nzh"]:, :].any() and not co[:, s["nzw"]:].any()
    if s["bdpcm"]:
        co = bdpcm(orc, co, s["vert"], rbits)
    orc.orc_dequant(co.ctypes.data, s["lw"], s["lh"], 0, 0, w - 1, h - 1, s["qp"], 1, 0, bd, rbits, None, 1, -1)
    return co


def residual_of(orc, s, bd, rbits=15):
    return oracle_residual(orc, s, bd, rbits) if s.get("ts") else tc.oracle_residual(orc, s, bd, rbits)


def oracle_walk(orc, pic, specs, offs, arena0, rbits=15):
    """What the stage leaves: (planes, arena, scale table or None) — inter_tb_cases.oracle_walk's order and tail (luma blocks, the table from
    the reconstructed luma, chroma blocks; add / scaled add / joint add / KEEP), the residual by residual_of: the specs may mix transform-skip
    blocks with the transformed blocks of inter_tb_cases."""
    bd, isz = pic.bd, pic.isz
    planes = [np.ascontiguousarray(p).copy() for p in pic.planes]
    arena = arena0.copy()
    table = None
    for ch in (0, 1):
        if ch == 1 and pic.model is not None:
            table = tc.oracle_scale_table(orc, pic, planes[0])
        for i, s in enumerate(specs):
            if (s["c_idx"] > 0) != ch or s.get("bad"):
                continue
            res = residual_of(orc, s, bd, rbits)
            w, h, c = 1 << s["lw"], 1 << s["lh"], s["c_idx"]
            if s["keep"]:
                arena[offs[i]:offs[i] + w * h] = res.ravel()
                continue
            for (plane, joint) in [(c, s["joint"] & 8)] + ([(3 - c, s["joint"])] if s["joint"] & 1 else []):
                pw = planes[plane].shape[1]
                dst = planes[plane].ctypes.data + (s["y0"] * pw + s["x0"]) * isz
                if joint & 8:
                    ux, uy = pic.unit_of(s, "cu")
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
    """The specs in record order (luma, then chroma; inside it by the class they are filed under; stable) and class_first[2][5]."""
    key = [(int(s.get("ch", s["c_idx"] > 0)), s.get("cls", area_class(s["lw"], s["lh"]))) for s in specs]
    order = sorted(range(len(specs)), key=lambda i: key[i])
    counts = np.zeros((2, NC), np.int64)
    for k in key:
        counts[k] += 1
    cum = np.concatenate([[0], np.cumsum(counts.ravel())])
    return [specs[i] for i in order], [[int(cum[ch * NC + k]) for k in range(NC + 1)] for ch in range(2)]


def records(pic, specs, offs):
    tus = batch.job_array(abi.TsTu, len(specs))
    for i, s in enumerate(specs):
        t = tus[i]
        t["coeff_off"], t["x0"], t["y0"] = offs[i] + s.get("off_add", 0), s["x0"], s["y0"]
        t["log2_w"], t["log2_h"], t["nzw"], t["nzh"], t["qp"] = s.get("rec_lw", s["lw"]), s.get("rec_lh", s["lh"]), s["nzw"], s["nzh"], s["qp"]
        (bx, by), (cx, cy) = pic.unit_of(s, "block"), pic.unit_of(s, "cu")
        assert 0 <= bx - cx <= 1 and 0 <= by - cy <= 1
        t["flags"] = (s["c_idx"] | (abi.TS_TU_BDPCM if s["bdpcm"] else 0) | (abi.TS_TU_VERTICAL if s["bdpcm"] and s["vert"] else 0) |
                      (abi.TS_TU_KEEP if s["keep"] else 0) | (abi.TS_TU_UNIT_DX if bx > cx else 0) | (abi.TS_TU_UNIT_DY if by > cy else 0) |
                      s.get("flags_or", 0))
        t["joint"] = s["joint"] | s.get("joint_or", 0)
        t["pad_"] = s.get("pad", 0)
    return tus


class Frame:
    """One run of vvc355_ts_tb_pass: records, arena, optional packed levels and the vvc355_ts_tb_frame (host copy + device copy).  With
    `shared` (an inter_tb_cases.Frame) the arena and the picture are that frame's: the two passes then work on one picture."""

    def __init__(self, pic, specs, class_first, offs, arena, rbits=15, packed=None, dpic=None, shared=None):
        self.pic, self.n, self.arena0 = pic, len(specs), arena
        self.dpic = shared.dpic if shared is not None else tc.DevicePicture(pic) if dpic is None else dpic
        self.d_tus = batch.DeviceBuffer.from_host(records(pic, specs, offs).view(np.uint8) if specs else np.zeros(16, np.uint8))
        self.d_arena = shared.d_arena if shared is not None else batch.DeviceBuffer.from_host(arena)
        f = abi.TsTbFrame()
        f.tus, f.coeffs, f.n_tus = self.d_tus.ptr, self.d_arena.ptr, self.n
        for c in range(3):
            f.plane[c], f.stride[c] = self.dpic.d_planes[c].ptr, self.dpic.strides[c]
        f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = pic.width, pic.height, pic.hs, pic.vs, pic.size_y, rbits, pic.bd
        f.scale_table = self.dpic.d_table.ptr if pic.model is not None else 0
        for ch in range(2):
            for k in range(NC + 1):
                f.class_first[ch][k] = class_first[ch][k]
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
        return dev.vvc355_ts_tb_pass(stream, self.d_f.ptr, ctypes.addressof(self.f), channels)

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
    """What the library offers these blocks without the entry, for KEEP blocks without BDPCM only: vvc355_levels_expand (a 48-byte
    vvc355_itx_job per block for the address and the shape, window w x h) + vvc355_dequant_batch (a 32-byte job per block, ts = 1)."""

    def __init__(self, pic, specs, offs, arena, rbits, packed):
        assert all(s["keep"] and not s["bdpcm"] for s in specs)
        self.n, self.arena0 = len(specs), arena
        self.d_arena = batch.DeviceBuffer.from_host(arena)
        jobs, dq = batch.job_array(abi.ItxJob, self.n), batch.job_array(abi.DequantJob, self.n)
        for i, s in enumerate(specs):
            w, h = 1 << s["lw"], 1 << s["lh"]
            j, d = jobs[i], dq[i]
            j["coeffs"] = d["coeffs"] = self.d_arena.ptr + offs[i] * 4
            j["log2_w"], j["log2_h"], j["nzw"], j["nzh"] = s["lw"], s["lh"], w, h
            d["log2_w"], d["log2_h"], d["max_x"], d["max_y"] = s["lw"], s["lh"], w - 1, h - 1
            d["qp"], d["ts"], d["bit_depth"], d["range"], d["log2_matrix_size"], d["dc"] = s["qp"], 1, pic.bd, rbits, 1, -1
        levels, lv = packed
        self.d_jobs, self.d_dq = batch.DeviceBuffer.from_host(jobs.view(np.uint8)), batch.DeviceBuffer.from_host(dq.view(np.uint8))
        self.d_lv, self.d_levels = batch.DeviceBuffer.from_host(lv.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
        self.job_bytes = jobs.nbytes + dq.nbytes

    def reset(self, dev):
        dev.vvc355_upload(self.d_arena.ptr, self.arena0.ctypes.data, self.arena0.nbytes)

    def expand(self, dev, stream=None):
        dev.vvc355_levels_expand(stream, self.d_jobs.ptr, self.d_lv.ptr, self.d_levels.ptr, self.n)

    def dequant(self, dev, stream=None):
        dev.vvc355_dequant_batch(stream, self.d_dq.ptr, self.n)

    def run(self, dev, stream=None):
        self.expand(dev, stream)
        self.dequant(dev, stream)

    def arena(self, dev):
        dev.vvc355_stream_sync(None)
        return self.d_arena.to_host(np.int32, self.arena0.shape)


def cells(pic, c_idx, size=32):
    ph, pw = pic.planes[c_idx].shape
    return [(x, y) for y in range(0, ph - size + 1, size) for x in range(0, pw - size + 1, size)]


def in_cell(rng, cell, lw, lh, size=32):
    """A position inside a size x size cell, a multiple of 4 samples (of 2 for a side of 2)."""
    w, h = 1 << lw, 1 << lh
    ax, ay = min(4, w), min(4, h)
    return cell[0] + int(rng.integers(0, (size - w) // ax + 1)) * ax, cell[1] + int(rng.integers(0, (size - h) // ay + 1)) * ay

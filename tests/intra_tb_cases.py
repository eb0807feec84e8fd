"""Transform blocks of intra coding units for vvc355_intra_tb_pass: block specs, their 16-byte records grouped by area class, the oracle chain
(orc_dequant -> orc_ilfnst_transform -> orc_derive_transform_type -> orc_itx, what itransform does for an intra coding unit) and the
device runs — the new entry, and the path it replaces (levels_expand -> lfnst_batch -> five itx_batch_lv launches).

A spec is a dict: lw, lh, c (int32 levels, shape (h, w)), nzw, nzh, c_idx, qp, dep, lfnst (bool), lfnst_idx, mode (pred_mode_intra), tu_flags,
mts_idx; optional cls (the class the record is filed under when it is not the one its area asks for)."""
import ctypes

import numpy as np

import levels_cases as lc
from ffvvc_amd import abi, batch

SENT = 0x7EADBEEF
GAP = 64                                   # sentinel words in front of, between and behind the blocks' arena slots
CLASS_CAP = (4, 6, 8, 10, 12)              # log2 of the largest area of class 0..4
# 6.5.2 up-right diagonal scan of a 4x4 block: (x, y) of scan position 0..15
DIAG4 = [(x, s - x) for s in range(7) for x in range(4) if 0 <= s - x < 4]
TU_INTRA_IMPLICIT = abi.TU_MTS_ENABLED | abi.TU_INTRA


def area_class(lw, lh):
    return next(k for k, cap in enumerate(CLASS_CAP) if lw + lh <= cap)


def lfnst_nz(w, h):
    """How many scan positions an LFNST block codes: 8 for 4x4 and 8x8, 16 otherwise."""
    return 8 if (w, h) in ((4, 4), (8, 8)) else 16


def lfnst_levels(rng, w, h, bits=6):
    """Levels in the first 8 / 16 positions of the 4x4 diagonal scan only: what a conformant stream codes for an LFNST block."""
    c = np.zeros((h, w), np.int32)
    for (x, y) in DIAG4[:lfnst_nz(w, h)]:
        c[y, x] = int(rng.integers(-(1 << bits), (1 << bits) + 1))
    if not c.any():
        c[0, 0] = 1
    return c


def spec(lw, lh, c, nzw, nzh, c_idx=0, qp=30, dep=0, lfnst=False, lfnst_idx=0, mode=0, tu_flags=TU_INTRA_IMPLICIT, mts_idx=0, cls=None):
    return dict(lw=lw, lh=lh, c=c, nzw=nzw, nzh=nzh, c_idx=c_idx, qp=qp, dep=dep, lfnst=lfnst, lfnst_idx=lfnst_idx, mode=mode,
                tu_flags=tu_flags, mts_idx=mts_idx, cls=area_class(lw, lh) if cls is None else cls)


def bind_oracle(orc):
    orc.orc_ilfnst_transform.restype = ctypes.c_int
    orc.orc_ilfnst_transform.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
    orc.orc_derive_transform_type.restype = ctypes.c_int
    orc.orc_derive_transform_type.argtypes = [ctypes.c_int] * 6


def oracle_block(orc, s, bd, rbits=15):
    """The residual of one block by the oracle chain."""
    w, h = 1 << s["lw"], 1 << s["lh"]
    co = np.ascontiguousarray(s["c"], np.int32).copy()
    nzw, nzh = s["nzw"], s["nzh"]
    if s["lfnst"]:
        orc.orc_dequant(co.ctypes.data, s["lw"], s["lh"], 0, 0, 3, 3, s["qp"], 0, s["dep"], bd, rbits, None, 1, -1)
        nzw = nzh = orc.orc_ilfnst_transform(co.ctypes.data, w, h, s["mode"], s["lfnst_idx"], rbits)
        assert nzw == (8 if (w >= 8 and h >= 8) else 4)
    else:
        orc.orc_dequant(co.ctypes.data, s["lw"], s["lh"], 0, 0, nzw - 1, nzh - 1, s["qp"], 0, s["dep"], bd, rbits, None, 1, -1)
    t = orc.orc_derive_transform_type(s["tu_flags"], s["mts_idx"], s["lfnst_idx"], s["c_idx"], w, h)
    assert orc.orc_itx(t & 15, t >> 4, s["lw"], s["lh"], co.ctypes.data, nzw, nzh, rbits, bd) == 0, (s["lw"], s["lh"], t)
    return co


def group_by_class(specs):
    """The specs in record order (stable by filed class) and class_first[6]."""
    order = sorted(range(len(specs)), key=lambda i: specs[i]["cls"])
    counts = np.bincount([specs[i]["cls"] for i in order], minlength=5)
    return [specs[i] for i in order], [0] + [int(v) for v in np.cumsum(counts)]


def arena_offsets(specs):
    """Element offset of every block's slot, GAP words between slots, and the arena length."""
    offs, off = [], GAP
    for s in specs:
        offs.append(off)
        off += (1 << (s["lw"] + s["lh"])) + GAP
    return offs, off


def records(specs, offs):
    tus = batch.job_array(abi.IntraTu, len(specs))
    for i, s in enumerate(specs):
        t = tus[i]
        t["coeff_off"], t["log2_w"], t["log2_h"], t["nzw"], t["nzh"] = offs[i], s["lw"], s["lh"], s["nzw"], s["nzh"]
        t["c_idx"], t["qp"], t["tu_flags"], t["mts_idx"], t["lfnst_idx"] = s["c_idx"], s["qp"], s["tu_flags"], s["mts_idx"], s["lfnst_idx"]
        t["flags"] = (abi.INTRA_TU_DEP_QUANT if s["dep"] else 0) | (abi.INTRA_TU_LFNST if s["lfnst"] else 0) | s.get("extra_flags", 0)
        t["pred_mode_intra"] = s["mode"]
    return tus


def start_arena(specs, offs, n, lv=None):
    """Sentinels everywhere; the levels of the blocks that are not packed (all of them without `lv`) in their slots."""
    arena = np.full(n, SENT, np.int32)
    for i, s in enumerate(specs):
        if lv is None or lv[i]["flags"] & abi.LEVELS_INT32:
            arena[offs[i]:offs[i] + s["c"].size] = s["c"].ravel()
    return arena


def expected_arena(orc, specs, offs, n, bd, rbits=15, skipped=()):
    """Sentinels + the oracle's residual of every block; blocks in `skipped` keep what the start arena held."""
    want = start_arena(specs, offs, n, None)
    for i, s in enumerate(specs):
        if i in skipped:
            continue
        want[offs[i]:offs[i] + s["c"].size] = oracle_block(orc, s, bd, rbits).ravel()
    return want


class Frame:
    """The device side of one run: records, arena, optional packed levels, and the vvc355_intra_tb_frame (host copy + device copy)."""

    def __init__(self, specs, class_first, offs, arena, bd, rbits=15, packed=None, launch_mode=0):
        self.n = len(specs)
        self.d_tus = batch.DeviceBuffer.from_host(records(specs, offs).view(np.uint8))
        self.arena0 = arena
        self.d_arena = batch.DeviceBuffer.from_host(arena)
        f = abi.IntraTbFrame()
        f.tus, f.coeffs, f.n_tus = self.d_tus.ptr, self.d_arena.ptr, self.n
        for k in range(6):
            f.class_first[k] = class_first[k]
        f.range, f.bd, f.launch_mode = rbits, bd, launch_mode
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

    def launch(self, dev, stream=None):
        return dev.vvc355_intra_tb_pass(stream, self.d_f.ptr, ctypes.addressof(self.f))

    def result(self, dev):
        dev.vvc355_stream_sync(None)
        return self.d_arena.to_host(np.int32, self.arena0.shape)


class OldPath:
    """The path the entry replaces, on the same records: 48-byte jobs (LFNST blocks: no fused scaling, window 4 / 8) and 32-byte LFNST jobs
    built on the host; vvc355_levels_expand of the packed LFNST blocks, vvc355_lfnst_batch, then one vvc355_itx_batch_lv per class."""

    def __init__(self, specs, class_first, offs, arena, bd, rbits, packed):
        levels, lv = packed
        n = len(specs)
        self.bd, self.class_first, self.arena0 = bd, class_first, arena
        self.d_arena = batch.DeviceBuffer.from_host(arena)
        itj = batch.job_array(abi.ItxJob, n)
        lf = [i for i, s in enumerate(specs) if s["lfnst"]]
        lfj = batch.job_array(abi.LfnstJob, len(lf))
        for i, s in enumerate(specs):
            j = itj[i]
            big = s["lw"] >= 3 and s["lh"] >= 3
            j["coeffs"], j["log2_w"], j["log2_h"], j["range"], j["bd"], j["store_coeffs"], j["c_idx"] = self.d_arena.ptr + offs[i] * 4, s["lw"], s["lh"], rbits, bd, 1, s["c_idx"]
            j["nzw"], j["nzh"] = ((8, 8) if big else (4, 4)) if s["lfnst"] else (s["nzw"], s["nzh"])
            j["dq_flags"] = 0 if s["lfnst"] else 1 | (s["dep"] << 1)
            j["dq_qp"], j["log2_matrix_size"], j["dc"] = s["qp"], 1, -1
            j["mts_flags"], j["tu_flags"], j["mts_idx"], j["lfnst_idx"] = abi.ITX_DERIVE_TYPE, s["tu_flags"], s["mts_idx"], s["lfnst_idx"]
        for k, i in enumerate(lf):
            s, l = specs[i], lfj[k]
            l["coeffs"], l["log2_w"], l["log2_h"], l["max_x"], l["max_y"] = itj[i]["coeffs"], s["lw"], s["lh"], 3, 3
            l["qp"], l["dequant"], l["dep_quant"], l["bit_depth"], l["range"], l["log2_matrix_size"], l["dc"] = s["qp"], 1, s["dep"], bd, rbits, 1, -1
            l["pred_mode_intra"], l["lfnst_idx"] = s["mode"], s["lfnst_idx"]
        lv_itx = lv.copy()
        lv_itx["flags"][lf] |= abi.LEVELS_INT32          # after expand + LFNST these blocks' coefficients are int32 in the arena
        self.n_lf = len(lf)
        self.jsz, self.lsz = itj.dtype.itemsize, lv.dtype.itemsize
        self.d_itj, self.d_lfj = batch.DeviceBuffer.from_host(itj.view(np.uint8)), batch.DeviceBuffer.from_host(lfj.view(np.uint8) if len(lf) else np.zeros(32, np.uint8))
        self.d_xj = batch.DeviceBuffer.from_host(itj[lf].view(np.uint8) if len(lf) else np.zeros(48, np.uint8))
        self.d_xlv = batch.DeviceBuffer.from_host(lv[lf].view(np.uint8) if len(lf) else np.zeros(16, np.uint8))
        self.d_lv, self.d_levels = batch.DeviceBuffer.from_host(lv_itx.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
        self.uploaded_bytes = n * self.jsz + len(lf) * lfj.dtype.itemsize

    def reset(self, dev):
        dev.vvc355_upload(self.d_arena.ptr, self.arena0.ctypes.data, self.arena0.nbytes)

    def launch(self, dev, stream=None):
        if self.n_lf:
            dev.vvc355_levels_expand(stream, self.d_xj.ptr, self.d_xlv.ptr, self.d_levels.ptr, self.n_lf)
            dev.vvc355_lfnst_batch(stream, self.d_lfj.ptr, self.n_lf)
        for k in range(5):
            first, cnt = self.class_first[k], self.class_first[k + 1] - self.class_first[k]
            if cnt:
                dev.vvc355_itx_batch_lv(stream, self.bd, self.d_itj.ptr + first * self.jsz, self.d_lv.ptr + first * self.lsz, self.d_levels.ptr,
                                        cnt, CLASS_CAP[k])
        return 0

    def result(self, dev):
        dev.vvc355_stream_sync(None)
        return self.d_arena.to_host(np.int32, self.arena0.shape)


def picture_specs(rng, tbs, lfnst_frac=0.2, max_nz=16):
    """The transform blocks of a recon_cases picture (work.tbs rows: c_idx, x0, y0, w, h, offset) with the draws of the bench's intra stage:
    LFNST on `lfnst_frac` of the luma blocks of at least 4x4 (levels in the 4x4 corner, index 1 / 2, mode -14..80), a scan window of up to
    16 x 16 elsewhere, Laplacian levels, qp 22..37, dep-quant on half of the blocks, implicit MTS."""
    out = []
    for (c_idx, _x, _y, w, h, _off) in tbs:
        lw, lh = int(w).bit_length() - 1, int(h).bit_length() - 1
        use = c_idx == 0 and w >= 4 and h >= 4 and rng.random() < lfnst_frac
        nzw, nzh = 1 + int(rng.random() * min(w, max_nz)), 1 + int(rng.random() * min(h, max_nz))
        qp, dep = int(rng.integers(22, 38)), int(rng.integers(0, 2))
        if use:
            c = np.zeros((h, w), np.int32)
            c[:4, :4] = lc.laplace_levels(rng, (4, 4))
            out.append(spec(lw, lh, c, min(w, 4), min(h, 4), 0, qp, dep, True, int(rng.integers(1, 3)), int(rng.integers(-14, 81))))
        else:
            out.append(spec(lw, lh, lc.windowed_block(rng, w, h, nzw, nzh), nzw, nzh, int(c_idx), qp, dep))
    return out

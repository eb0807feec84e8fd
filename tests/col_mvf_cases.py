"""Cases, expectation and device plumbing for vvc355_col_mvf_pass (the hand-back of collocated motion), used by tests/test_col_mvf_cpu.py,
tests/test_col_mvf_gpu.py and tools/col_mvf_time.py.

The expectation is numpy, written from the header's packing and from H.266 clause 8.5.2.15 (temporal motion buffer compression):
  s = mvCol >> 17; f = Floor(Log2((mvCol ^ s) | 31)) - 4; mask = (-1 << f) >> 1; round = (1 << f) >> 2; mvCol = (mvCol + round) & mask
test_col_mvf_cpu.py pins it to a scalar loop over the whole range and to values worked by hand.

The DMVR pictures are three of ref_inter_cases' regular pictures, one per bit depth, whose tab_dmvr_mvf tests/golden/ref_inter.json pins to
the reference, and the directed picture T0.  The listed pictures split CTUs in halves and quarters only, so their sub-blocks of 8 or 16 a
side all start on the 8-sample grid; T0 has what a ternary split gives: DMVR units behind a 4-wide (or under a 4-high) neighbour, which
start at 4 mod 8 and cover ONE grid column (row) although they are 8 wide (high)."""
import ctypes

import numpy as np

import affine_gpm_cases as agc
import bipred_cases as bc
import inter_frame_cases as ifc
import ref_inter_cases as ic
from ffvvc_amd import abi, batch

SEED = 0xC01F0000
SENTINEL = 0xC7
SLACK = 64                                     # sentinel bytes in front of and behind the `col` array (a multiple of 16)
MV_BITS, MV_MASK, KEEP_MASK = 19, 0x7FFFF, 0xFFF80000
ENTRY = ctypes.sizeof(abi.ColMv)

DIRECTED = [(4, 4, 0, 0), (8, 8, 0, 0), (12, 8, 0, 0), (520, 8, 0, 0), (1032, 24, 0, 0), (136, 72, 41, 23)]      # width, height, mvf_stride, col_stride (0: as needed)
LISTED_DMVR = ["R1", "R0", "R2"]               # 8, 10 and 12 bit
DMVR_PICTURES = LISTED_DMVR + ["T0"]


def grid(width, height):
    return (width + 7) // 8, (height + 7) // 8


# ---------------------------------------------------------------------------------------------------------------- the expectation

def compress(v):
    """Clause 8.5.2.15 on every element of an integer array."""
    v = np.asarray(v, np.int64)
    s = v >> 17
    f = np.frexp(((v ^ s) | 31).astype(np.float64))[1] - 1 - 4            # Floor(Log2(.)) - 4: frexp's exponent is exact
    mask = (-np.left_shift(np.int64(1), f)) >> 1
    rnd = np.left_shift(np.int64(1), f) >> 2
    return (v + rnd) & mask


def compress_scalar(v):
    """The same on one Python int, step by step."""
    s = v >> 17
    f = ((v ^ s) | 31).bit_length() - 1 - 4
    mask = (-1 << f) >> 1
    rnd = (1 << f) >> 2
    return (v + rnd) & mask


def pack(mvf, do_compress):
    """uint32 [gy][gx][list][x, y] of an MvField table [row][column] (ifc.MVF_DT), as the header states the entry."""
    m = mvf[0::2, 0::2]
    pf = m["pred_flag"].astype(np.uint32) & 3
    mv = m["mv"].astype(np.int64)
    if do_compress:
        mv = compress(mv)
    out = np.zeros(m.shape + (2, 2), np.uint32)
    for l in range(2):
        used = ((pf >> l) & 1).astype(bool)
        ref = m["ref_idx"][..., l].astype(np.int64) & 0x1F
        out[..., l, 0] = np.where(used, (mv[..., l, 0] & MV_MASK) | (ref << MV_BITS), 0)
        out[..., l, 1] = np.where(used, mv[..., l, 1] & MV_MASK, 0)
    out[..., 0, 1] |= pf << MV_BITS
    return out


def unpack(col):
    """(mv int32 [...][list][x, y], ref_idx int8 [...][list], pred_flag uint8 [...]) of packed entries [...][list][x, y]."""
    col = np.asarray(col, np.uint32)
    pf = ((col[..., 0, 1] >> MV_BITS) & 3).astype(np.uint8)
    used = ((pf[..., None] >> np.arange(2)) & 1).astype(bool)
    v = (col & MV_MASK).astype(np.int64)
    mv = np.where(used[..., None], v - ((v & (1 << (MV_BITS - 1))) << 1), 0).astype(np.int32)
    ref = np.where(used, (col[..., 0] >> MV_BITS) & 0x1F, -1).astype(np.int8)
    return mv, ref, pf


def job_ok(x, y, w, h, width, height):
    return not (x % 4 or y % 4 or x < 0 or y < 0 or w not in (8, 16) or h not in (8, 16) or x + w > width or y + h > height)


def overlay(col, jobs, recs, width, height, do_compress):
    """set_dmvr_info on the entries: `jobs` (x, y, w, h, dmvr) per luma job, `recs` its record's mv[4]."""
    col = col.copy()
    for (x, y, w, h, dmvr), r in zip(jobs, recs):
        if not dmvr or not job_ok(x, y, w, h, width, height):
            continue
        mv = np.array([int(v) for v in r[:4]], np.int64).reshape(2, 2)
        if do_compress:
            mv = compress(mv)
        for gy in range((y + 7) // 8, (y + h + 7) // 8):
            for gx in range((x + 7) // 8, (x + w + 7) // 8):
                pf = (int(col[gy, gx, 0, 1]) >> MV_BITS) & 3
                for l in range(2):
                    if (pf >> l) & 1:
                        col[gy, gx, l] = (col[gy, gx, l] & KEEP_MASK) | (mv[l] & MV_MASK).astype(np.uint32)
    return col


def jobs_of(jl):
    """(x, y, w, h, dmvr) of a structured array of vvc355_bipred_job."""
    return [(int(j["x"]), int(j["y"]), int(j["w"]), int(j["h"]), int(j["dmvr"])) for j in jl]


# ---------------------------------------------------------------------------------------------------------------- tables

def directed_table(seed, width, height, mvf_stride=0, shift=0):
    """An MvField table [height / 4][mvf_stride] of noise — every byte of it, pad bytes, the odd positions and the row padding included — in
    which the entries at the even positions have pred_flag (gx + gy + shift) & 3, motion of the lists they use anywhere in 18 bits signed
    with the ends of the range among it, and ref_idx 0..15 there.  The motion and ref_idx of the lists they do not use stay noise."""
    rng = np.random.default_rng([SEED, seed, width, height, shift])
    th, tw = height // 4, mvf_stride or width // 4
    t = rng.integers(0, 256, size=(th, tw, ifc.MVF_DT.itemsize), dtype=np.int64).astype(np.uint8).view(ifc.MVF_DT).reshape(th, tw)
    m = t[0::2, 0:(width // 4):2]
    gy, gx = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    pf = ((gx + gy + shift) & 3).astype(np.uint8)
    m["pred_flag"] = pf
    for l in range(2):
        used = ((pf >> l) & 1).astype(bool)
        mv = rng.integers(-(1 << 17), 1 << 17, size=m.shape + (2,))
        ends = rng.random(m.shape) < 0.2
        mv[ends] = rng.choice([-(1 << 17), (1 << 17) - 1, -1, 0, 31, -32, 65], size=(int(ends.sum()), 2))
        m["mv"][:, :, l] = np.where(used[..., None], mv, m["mv"][:, :, l])
        m["ref_idx"][:, :, l] = np.where(used, rng.integers(0, 16, size=m.shape), m["ref_idx"][:, :, l])
    return t


def whole_range_table():
    """2048x2048: the 65 536 entries at the even positions carry every value of [-2^17, 2^17 - 1] once, across the four components, in a
    shuffled order; bi-predicted, ref_idx 0..15; zeros at the odd positions."""
    rng = np.random.default_rng([SEED, 2048])
    t = np.zeros((512, 512), ifc.MVF_DT)
    m = t[0::2, 0::2]
    m["mv"] = rng.permutation(np.arange(-(1 << 17), 1 << 17)).reshape(256, 256, 2, 2)
    m["pred_flag"] = 3
    m["ref_idx"] = rng.integers(0, 16, size=(256, 256, 2))
    return t


# ---------------------------------------------------------------------------------------------------------------- the directed picture

_made = {}


def offgrid_picture():
    """T0: one 64x64 CTU, 10 bit 4:2:0, with the units ternary splits give (vvc_ctu.c: SPLIT_TT_VER / _HOR cut 16 into 4, 8, 4 and 32 into
    8, 16, 8): DMVR units of 8x16 at x = 4 and x = 36, of 16x8 at y = 4 and y = 36, a 16-wide one at x = 40 and an aligned 16x16, between
    4-wide uni-predicted neighbours; the rest of the CTU stays without motion (pred_flag 0)."""
    if "T0" not in _made:
        rng = np.random.default_rng(SEED + 40)
        p = ic.Picture.__new__(ic.Picture)
        p.name, p.bd, p.idc, p.ctb_log2, p.kinds = "T0", 10, 1, 6, "R"
        p.width, p.height = 64, 64
        p.hs, p.vs = ic.FMT[p.idc]
        p.chroma, p.isz, p.n_comp = True, 2, 3
        p.dims = [(64, 64), (32, 32), (32, 32)]
        p.sentinel = (1 << p.bd) // 3
        p.ncx, p.ncy, p.ctu_slice = 1, 1, [0]
        p.slices = ic.make_slices(rng)
        p.mvf = np.zeros((16, 16), ifc.MVF_DT)
        p.covered = np.zeros((64, 64), bool)
        p.units = []
        base = [bc.smooth_picture(rng, ph, pw, p.bd) for (pw, ph) in p.dims]
        p.refs = [[[bc.shifted(base[c], ic.ref_shift(l, r)[0] >> (p.hs if c else 0), ic.ref_shift(l, r)[1] >> (p.vs if c else 0)) for c in range(3)]
                   for r in range(2)] for l in range(2)]
        p.lut = np.sort(np.random.default_rng(0x10C5 + p.bd).integers(0, 1 << p.bd, size=1 << p.bd)).astype(ic.px(p.bd))
        p._part = 0
        units = [(0, 0, 4, 16, None), (4, 0, 8, 16, "d"), (12, 0, 4, 16, None),                  # 16x16 cut vertically
                 (16, 0, 16, 4, None), (16, 4, 16, 8, "d"), (16, 12, 16, 4, None),               # 16x16 cut horizontally
                 (32, 0, 8, 32, "d"), (40, 0, 16, 32, "db"), (56, 0, 8, 32, "d"),                # 32x32 cut vertically
                 (0, 16, 16, 16, "d"),
                 (0, 32, 16, 4, None), (0, 36, 16, 8, "db"), (0, 44, 16, 4, None),
                 (32, 32, 4, 32, None), (36, 32, 8, 32, "db"), (44, 32, 4, 32, None)]             # 16x32 cut vertically
        pus = []
        for (x, y, w, h, forced) in units:
            p.covered[y:y + h, x:x + w] = True
            p.units.append(("R", x, y, w, h))
            pus.append(p._regular(rng, x, y, w, h, 0, 20 * 16, forced))
        p._finish(pus, [], [])
        _made["T0"] = p
    return _made["T0"]


def dmvr_picture(name):
    return offgrid_picture() if name == "T0" else ic.picture(name)


def oracle_run(orc, name):
    """The oracle's run of the picture, once per process: .dmvr is tab_dmvr_mvf, .jl / .rec the luma jobs and their records."""
    if ("orc", name) not in _made:
        _made[("orc", name)] = ic.run_picture(orc, "orc", dmvr_picture(name))
    return _made[("orc", name)]


def refined_points(pic, run):
    """[(gx, gy, job)] of the grid points inside a DMVR sub-block whose refined vector differs from the table's, and the set of
    (x % 8, y % 8) at which DMVR sub-blocks start."""
    points, starts = [], set()
    for i, (x, y, w, h, dmvr) in enumerate(jobs_of(run.jl)):
        if not dmvr:
            continue
        assert job_ok(x, y, w, h, pic.width, pic.height)
        starts.add((x % 8, y % 8))
        if np.array_equal(run.rec[i][:4], pic.mvf[y >> 2, x >> 2]["mv"].reshape(-1)):
            continue
        points += [(gx, gy, i) for gy in range((y + 7) // 8, (y + h + 7) // 8) for gx in range((x + 7) // 8, (x + w + 7) // 8)]
    return points, starts


# ---------------------------------------------------------------------------------------------------------------- frames and device plumbing

def frame_of(width, height, mvf, col, mvf_stride=0, col_stride=0, flags=0, jobs=0, records=0, n_jobs=0):
    f = abi.ColMvfFrame()
    f.mvf, f.col, f.jobs_luma, f.records = mvf, col, jobs, records
    f.width, f.height, f.mvf_stride, f.col_stride = width, height, mvf_stride or width // 4, col_stride or grid(width, height)[0]
    f.n_jobs, f.flags = n_jobs, flags
    return f


def valid_frame(**kw):
    """A host frame with made-up addresses that the pass accepts, for the refusals (nothing may be launched)."""
    args = dict(width=416, height=240, mvf=0x100000, col=0x800000)
    args.update(kw)
    return frame_of(**args)


def up(a):
    a = np.ascontiguousarray(a)
    return batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a)


class ColRun:
    """One frame on a device table: a `col` allocation filled with SENTINEL, the array SLACK bytes in, rows of `col_stride` entries of which
    the last is cut after its ceil(width / 8) entries, SLACK bytes behind."""

    def __init__(self, lib, width, height, mvf_ptr, mvf_stride=0, col_stride=0, flags=0, jobs=0, records=0, n_jobs=0):
        self.lib, self.width, self.height = lib, width, height
        self.gw, self.gh = grid(width, height)
        self.col_stride = col_stride or self.gw
        self.image = np.full(SLACK + ((self.gh - 1) * self.col_stride + self.gw) * ENTRY + SLACK, SENTINEL, np.uint8)
        self.buf = batch.DeviceBuffer.from_host(self.image)
        assert self.buf.ptr % 16 == 0
        self.frame = frame_of(width, height, mvf_ptr, self.buf.ptr + SLACK, mvf_stride, self.col_stride, flags, jobs, records, n_jobs)
        self.d_frame = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.frame), np.uint8))

    def issue(self, stream=None):
        return self.lib.vvc355_col_mvf_pass(stream, self.d_frame.ptr, ctypes.addressof(self.frame))

    def reset(self):
        self.lib.vvc355_upload(self.buf.ptr, self.image.ctypes.data, self.image.nbytes)

    def download(self):
        return self.buf.to_host(np.uint8, self.image.shape)

    def expected_image(self, col):
        """Every byte of the allocation after the pass, for entries `col` [gh][gw][2][2]: the rows' entries, SENTINEL everywhere else."""
        assert col.shape == (self.gh, self.gw, 2, 2) and col.dtype == np.uint32
        img = self.image.copy()
        rows = np.ascontiguousarray(col).view(np.uint8).reshape(self.gh, self.gw * ENTRY)
        for gy in range(self.gh):
            at = SLACK + gy * self.col_stride * ENTRY
            img[at:at + self.gw * ENTRY] = rows[gy]
        return img

    def entries(self, image=None):
        """[gh][gw][2][2] out of the allocation's bytes."""
        img = self.download() if image is None else image
        rows = [img[SLACK + gy * self.col_stride * ENTRY:SLACK + (gy * self.col_stride + self.gw) * ENTRY] for gy in range(self.gh)]
        return np.stack(rows).view("<u4").reshape(self.gh, self.gw, 2, 2)

    def mismatch(self, col):
        """'' where the allocation holds exactly what it must, otherwise where the first difference lies."""
        got, want = self.download(), self.expected_image(col)
        if np.array_equal(got, want):
            return ""
        at = int(np.flatnonzero(got != want)[0])
        e, b = divmod(at - SLACK, ENTRY)
        return (f"{self.width}x{self.height}, flags {self.frame.flags}, {self.frame.n_jobs} jobs: byte {at} of the allocation (row {e // self.col_stride}, entry "
                f"{e % self.col_stride} of {self.gw} at stride {self.col_stride}, byte {b}) is {got[at]:#x}, expected {want[at]:#x}; {int((got != want).sum())} bytes differ")

    def run(self, col, stream=None):
        assert self.issue(stream) == 0
        self.lib.vvc355_stream_sync(stream)
        assert self.lib.vvc355_last_error() == 0
        return self.mismatch(col)


class InterRun:
    """A DMVR picture's regular units through vvc355_inter_frame_pass on the device, with or without a full dmvr_mvf table; what the
    hand-back reads stays alive in the object: d_mvf (unrefined), d_dmvr (tab_dmvr_mvf, with_table only), d_jl, d_rec."""

    def __init__(self, lib, pic, with_table):
        self.pic = pic
        dt = ic.px(pic.bd)
        pitches = [batch.plane_pitch(d[0], pic.isz) for d in pic.dims]
        d_dst = [up(batch.to_pitched(np.full((ph, pw), pic.sentinel, dt))) for (pw, ph) in pic.dims[:pic.n_comp]]
        d_ref = [[[up(batch.to_pitched(pic.refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
        reft = agc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], [[pitches] * 2] * 2)
        self.d_mvf, self.d_dmvr = up(pic.mvf), (up(pic.mvf) if with_table else None)          # tab_dmvr_mvf as the parser leaves it: a copy
        job = agc.BIPRED_JOB_DT.itemsize
        self.d_jl, d_jc, self.d_rec = (batch.DeviceBuffer(max(n, 64)) for n in (pic.n_jobs * job, 2 * pic.n_jobs * job, pic.n_jobs * 32))
        self.keep = [d_dst, d_ref, d_jc, up(np.frombuffer(bytes(reft), np.uint8)), up(np.frombuffer(bytes(pic.slices), np.uint8)), up(pic.lut), up(pic.pus)]
        f = pic.frame([b.ptr for b in d_dst] + [0] * (3 - pic.n_comp), pitches, self.d_mvf.ptr, self.keep[3].ptr, self.keep[4].ptr, self.keep[5].ptr,
                      self.keep[6].ptr, self.d_jl.ptr, d_jc.ptr, self.d_rec.ptr, self.d_dmvr.ptr if with_table else 0)
        self.keep += [f, up(np.frombuffer(bytes(f), np.uint8))]
        self.issue = lambda stream=None: lib.vvc355_inter_frame_pass(stream, pic.bd, self.keep[-1].ptr, ctypes.addressof(f))

    def hand_back(self, lib, flags, col_stride=0):
        """The ColRun that reads this run's tables: the full table where there is one, otherwise the unrefined one plus jobs and records."""
        p = self.pic
        if self.d_dmvr is not None:
            return ColRun(lib, p.width, p.height, self.d_dmvr.ptr, 0, col_stride, flags)
        return ColRun(lib, p.width, p.height, self.d_mvf.ptr, 0, col_stride, flags, self.d_jl.ptr, self.d_rec.ptr, p.n_jobs)

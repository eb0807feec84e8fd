"""GPU parity of vvc355_inter_frame_build alone: both job arrays byte for byte, padding included, against orc_inter_frame_build.

The kernel gives a lane to a job, stages the jobs of a workgroup's 64 coding units as rows in LDS and copies them out as contiguous
ranges, in chunks of 64 jobs.  The oracle runs on a host twin of the frame: host pointers for mvf, pus, slices, refs and the job
arrays, while dst, records, lmcs_fwd_lut and the planes of the reference table hold the device's numeric addresses — the build only does
arithmetic on those, so the expected bytes are the device's.  Every device array ends in 4 KB of 0xA5 that must survive."""
import ctypes

import numpy as np
import pytest

import inter_frame_cases as ifc
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu
TAIL = 4096
JOB = ctypes.sizeof(abi.BipredJob)


class Guarded:
    """A device array followed by TAIL bytes of 0xA5."""

    def __init__(self, host_bytes):
        self.n = len(host_bytes)
        self.buf = batch.DeviceBuffer.from_host(np.concatenate([np.frombuffer(host_bytes, np.uint8), np.full(TAIL, 0xA5, np.uint8)]))
        self.ptr = self.buf.ptr

    def body(self):
        return self.buf.to_host(np.uint8, (self.n + TAIL,))[:self.n]

    def tail_intact(self):
        return bool((self.buf.to_host(np.uint8, (self.n + TAIL,))[self.n:] == 0xA5).all())


class Grid16:
    """width x height in 16x16 bi-predicted units of one job each, DMVR and BDOF on: the shape of the benchmark's picture."""

    def __init__(self, rng, width, height):
        self.width, self.height = width, height
        self.mvf = np.zeros((height // 4, width // 4), ifc.MVF_DT)
        self.mvf["mv"] = np.repeat(np.repeat(rng.integers(-300, 301, size=(height // 16, width // 16, 2, 2)), 4, axis=0), 4, axis=1)
        self.mvf["ref_idx"] = np.repeat(np.repeat(rng.integers(0, 2, size=(height // 16, width // 16, 2)), 4, axis=0), 4, axis=1)
        self.mvf["pred_flag"] = 3
        self.pus = np.array([(x, y, 16, 16, 1, 1, 1, 1, 0, 0, 0, 0, 0) for y in range(0, height, 16) for x in range(0, width, 16)], dtype=ifc.PU_DT)
        self.pus["first_job"] = np.arange(len(self.pus))
        self.n_jobs = len(self.pus)
        self.slices = (abi.InterSlice * 2)()
        self.slices[0].lmcs_used = 1


def run_build(dev, orc, work, bd, hs, vs, chroma_format_idc=1):
    """The device's and the oracle's (jobs_luma, jobs_chroma) as bytes; the 0xA5 tails of every device array are checked here."""
    orc.orc_inter_frame_build.argtypes = [ctypes.POINTER(abi.InterFrame)]
    orc.orc_inter_frame_build.restype = None
    isz = 1 if bd == 8 else 2
    w, h, n = work.width, work.height, work.n_jobs
    dims = [(w, h), (w >> hs, h >> vs), (w >> hs, h >> vs)]
    pitches = [batch.plane_pitch(d[0], isz) for d in dims]
    # planes are only addresses to the build: carve them out of one allocation
    sizes = [pitches[c] * dims[c][1] for c in range(3)]
    arena = Guarded(bytes(5 * sum(sizes) + (isz << bd)))
    at, dst = arena.ptr, []
    for c in range(3):
        dst.append(at); at += sizes[c]
    refs = (abi.RefPic * 32)()
    for l in range(2):
        for r in range(2):
            for c in range(3):
                refs[l * 16 + r].plane[c], refs[l * 16 + r].stride[c] = at, pitches[c]
                at += sizes[c]
    lut = at
    g_mvf, g_pus = Guarded(work.mvf.tobytes()), Guarded(work.pus.tobytes())
    g_sl, g_refs = Guarded(bytes(work.slices)), Guarded(bytes(refs))
    g_rec = Guarded(bytes(32 * n))
    g_jl, g_jc = Guarded(b"\xA5" * (JOB * n)), Guarded(b"\xA5" * (2 * JOB * n))
    h_jl, h_jc = np.full(JOB * n, 0xA5, np.uint8), np.full(2 * JOB * n, 0xA5, np.uint8)

    def frame(mvf, refs_, pus, slices, jl, jc):
        f = abi.InterFrame()
        for c in range(3):
            f.dst[c], f.dst_stride[c] = dst[c], pitches[c]
        f.mvf, f.refs, f.pus, f.slices, f.jobs_luma, f.jobs_chroma, f.records = mvf, refs_, pus, slices, jl, jc, g_rec.ptr
        f.lmcs_fwd_lut = lut
        f.mvf_stride, f.n_pus, f.n_jobs, f.width, f.height = w // 4, len(work.pus), n, w, h
        f.hs, f.vs, f.chroma_format_idc, f.pixel_shift = hs, vs, chroma_format_idc, int(isz == 2)
        return f

    hf = frame(work.mvf.ctypes.data, ctypes.addressof(refs), work.pus.ctypes.data, ctypes.addressof(work.slices), h_jl.ctypes.data, h_jc.ctypes.data)
    orc.orc_inter_frame_build(ctypes.byref(hf))
    df = frame(g_mvf.ptr, g_refs.ptr, g_pus.ptr, g_sl.ptr, g_jl.ptr, g_jc.ptr)
    d_f = Guarded(bytes(df))
    dev.vvc355_inter_frame_build(None, d_f.ptr, ctypes.addressof(df))
    dev.vvc355_stream_sync(None)
    for name, g in (("planes", arena), ("mvf", g_mvf), ("pus", g_pus), ("slices", g_sl), ("refs", g_refs), ("records", g_rec), ("jobs_luma", g_jl),
                    ("jobs_chroma", g_jc), ("frame", d_f)):
        assert g.tail_intact(), f"the 0xA5 tail of {name} was written"
    assert not g_rec.body().any() and np.array_equal(g_pus.body(), np.frombuffer(work.pus.tobytes(), np.uint8))
    return (g_jl.body(), g_jc.body()), (h_jl, h_jc)


def assert_same_jobs(got, want, n_jobs):
    for name, g, e in zip(("jobs_luma", "jobs_chroma"), got, want):
        bad = np.flatnonzero(g != e)
        assert len(bad) == 0, f"{name}: {len(bad)} bytes differ, first in job {bad[0] // JOB} at byte {bad[0] % JOB}"
    assert not (want[0].reshape(n_jobs, JOB) == 0xA5).all(axis=1).any()          # the oracle wrote every job


def counts_of(work):
    return np.array([ifc.n_jobs_of(p["cb_width"], p["cb_height"], p["num_sb_x"], p["num_sb_y"]) for p in work.pus], np.int64)


@pytest.mark.parametrize("bd,fmt,w,h", [(10, (1, 1), 256, 192), (10, (1, 1), 320, 320), (12, (1, 0), 128, 128), (8, (1, 1), 128, 128)])
def test_inter_build_mixed_units(dev, orc, bd, fmt, w, h):
    """Mixed units, 8x8 sub-block merge, 16x16 tiles, two slices with weights; at 320x320 five workgroups with several chunks each."""
    work = ifc.InterWork(np.random.default_rng(0xB01D + bd + w), w, h)
    counts = counts_of(work)
    assert counts.max() >= 16 and (counts == 1).any()
    if w == 320:
        # the first workgroup's 64 units have more than 64 jobs, and one of them straddles the chunk boundary; more workgroups follow
        first = work.pus["first_job"].astype(np.int64)[:64]
        assert len(work.pus) > 256 and ((first < 64) & (first + counts[:64] > 64)).any()
    got, want = run_build(dev, orc, work, bd, *fmt)
    assert_same_jobs(got, want, work.n_jobs)


def test_inter_build_single_job_units(dev, orc):
    """272 single-job 16x16 bi-predicted units: four full workgroups and a partial one."""
    work = Grid16(np.random.default_rng(0xB01E), 272, 256)
    assert len(work.pus) == 272 and work.n_jobs == 272
    got, want = run_build(dev, orc, work, 10, 1, 1)
    assert_same_jobs(got, want, work.n_jobs)


def test_inter_build_no_chroma(dev, orc):
    """chroma_format_idc 0: jobs_chroma keeps its 0xA5 fill."""
    work = ifc.InterWork(np.random.default_rng(0xB01F), 256, 192)
    got, want = run_build(dev, orc, work, 10, 0, 0, chroma_format_idc=0)
    assert_same_jobs(got, want, work.n_jobs)
    assert (got[1] == 0xA5).all()


def test_inter_build_reordered_list(dev, orc):
    """The unit list reversed with its first_job values kept: no running sum, so the workgroup takes the lane-per-unit path."""
    work = ifc.InterWork(np.random.default_rng(0xB01D + 10 + 256), 256, 192)
    work.pus = np.ascontiguousarray(work.pus[::-1])
    assert (np.diff(work.pus["first_job"].astype(np.int64)) < 0).all()
    got, want = run_build(dev, orc, work, 10, 1, 1)
    assert_same_jobs(got, want, work.n_jobs)

"""GPU parity of vvc355_itx_frame_build alone: the transform jobs and the chroma residual jobs byte for byte, padding included.

The kernel stages a workgroup's 256 jobs as rows in LDS and copies them out as one contiguous range per array.  The expected arrays are
written here in numpy from the field definitions of vvc355_itx_job / vvc355_lmcs_resid_job (include/vvc_mi355.h).  Both device arrays
are pre-filled with 0xA5 and end in 4 KB of 0xA5 that must survive: a record count that is no multiple of the workgroup must not write
past the arrays, and a record without flags bit 6 still gets a residual job of zeros."""
import ctypes

import numpy as np
import pytest

from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu
TAIL = 4096
PW, PH, SIZE_Y, TU_FLAGS = 256, 128, 64, 5


def records(rng, n):
    """Random shapes from 4x4 to 64x64 in all three components (4:2:0), every combination of the flag bits 1 .. 64."""
    tus = np.zeros(n, np.dtype(abi.ItxTu, align=True))
    c = rng.integers(0, 3, size=n)
    lw, lh = rng.integers(2, 7, size=n), rng.integers(2, 7, size=n)
    cw, ch = np.where(c > 0, PW // 2, PW), np.where(c > 0, PH // 2, PH)
    tus["c_idx"], tus["log2_w"], tus["log2_h"] = c, lw, lh
    tus["x0"] = rng.integers(0, (cw >> lw)) << lw
    tus["y0"] = rng.integers(0, (ch >> lh)) << lh
    tus["nzw"], tus["nzh"] = rng.integers(1, (1 << np.minimum(lw, 5)) + 1), rng.integers(1, (1 << np.minimum(lh, 5)) + 1)
    tus["qp"], tus["tr"] = rng.integers(22, 40, size=n), rng.integers(0, 3, size=n) | rng.integers(0, 3, size=n) << 4
    tus["flags"] = rng.integers(0, 128, size=n)
    tus["coeff_off"] = np.concatenate(([0], np.cumsum(1 << (lw + lh))[:-1]))
    return tus


def expected(tus, f):
    """(jobs, resid jobs) as the header defines them; addresses are the frame's numbers."""
    n = len(tus)
    j, r = batch.job_array(abi.ItxJob, n), batch.job_array(abi.LmcsResidJob, n)
    c = tus["c_idx"].astype(np.int64)
    plane = np.array([f.plane[k] for k in range(3)], np.uint64)[c]
    stride = np.array([f.stride[k] for k in range(3)], np.int64)[c]
    flags = tus["flags"].astype(np.int64)
    keep = (flags & 4) != 0
    at = plane + (tus["y0"].astype(np.int64) * stride + (tus["x0"].astype(np.int64) << f.pixel_shift)).astype(np.uint64)
    j["coeffs"] = np.uint64(f.coeffs) + tus["coeff_off"].astype(np.uint64) * np.uint64(4)
    j["dst"], j["dst_stride"] = np.where(keep, np.uint64(0), at), stride
    j["trh"], j["trv"] = tus["tr"] & 15, tus["tr"] >> 4
    for k in ("log2_w", "log2_h", "nzw", "nzh", "c_idx"):
        j[k] = tus[k]
    j["range"], j["bd"], j["tu_flags"] = f.range, f.bd, f.tu_flags
    j["store_coeffs"], j["dq_flags"], j["dq_qp"] = keep, flags & 3, tus["qp"]
    j["log2_matrix_size"], j["dc"] = 1, -1
    j["mts_flags"] = (flags & 8) != 0
    m = (flags & 64) != 0
    x_vpdu = (tus["x0"].astype(np.int64) << np.where(c > 0, f.hs, 0)) & ~(SIZE_Y - 1)
    y_vpdu = (tus["y0"].astype(np.int64) << np.where(c > 0, f.vs, 0)) & ~(SIZE_Y - 1)
    r["dst"], r["resid"], r["dst_stride"], r["luma_stride"] = at, j["coeffs"], stride, f.stride[0]
    r["w"], r["h"] = 1 << tus["log2_w"].astype(np.int64), 1 << tus["log2_h"].astype(np.int64)
    r["x_vpdu"], r["y_vpdu"], r["pic_w"], r["pic_h"], r["size_y"] = x_vpdu, y_vpdu, f.width, f.height, SIZE_Y
    r["avail_l"], r["avail_t"] = (flags >> 4) & 1, (flags >> 5) & 1
    if f.scale_table:
        ux = (f.width + SIZE_Y - 1) // SIZE_Y
        r["luma"], r["joint"] = np.uint64(f.scale_table) + ((y_vpdu // SIZE_Y * ux + x_vpdu // SIZE_Y) * 2).astype(np.uint64), 8 | 16
    else:
        r["luma"], r["joint"] = f.plane[0], 8
    r[~m] = np.zeros((), r.dtype)
    return j, r


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("mode", ["jobs", "resid", "resid_table"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_itx_build_stores(dev, n, mode, bd):
    rng = np.random.default_rng(0x17B0 + 3 * n + bd)
    isz = 1 if bd == 8 else 2
    tus = records(rng, n)
    jsz, rsz = ctypes.sizeof(abi.ItxJob), ctypes.sizeof(abi.LmcsResidJob)
    d_tus = batch.DeviceBuffer.from_host(np.concatenate([tus.view(np.uint8), np.full(TAIL, 0xA5, np.uint8)]))
    d_jobs = batch.DeviceBuffer.from_host(np.full(n * jsz + TAIL, 0xA5, np.uint8))
    d_rjobs = batch.DeviceBuffer.from_host(np.full(n * rsz + TAIL, 0xA5, np.uint8))
    # planes, coefficient arena and scale table are only addresses to the build
    pitches = [batch.plane_pitch(PW, isz), batch.plane_pitch(PW // 2, isz), batch.plane_pitch(PW // 2, isz)]
    d_arena = batch.DeviceBuffer(pitches[0] * PH + 2 * pitches[1] * (PH // 2) + 4096)
    f = abi.ItxFrame()
    f.tus, f.jobs, f.coeffs, f.n_tus = d_tus.ptr, d_jobs.ptr, d_arena.ptr + 0x100000, n
    f.plane[0], f.plane[1], f.plane[2] = d_arena.ptr, d_arena.ptr + pitches[0] * PH, d_arena.ptr + pitches[0] * PH + pitches[1] * (PH // 2)
    for c in range(3):
        f.stride[c] = pitches[c]
    f.range, f.bd, f.pixel_shift, f.tu_flags = 15, bd, int(isz == 2), TU_FLAGS
    f.width, f.height, f.hs, f.vs, f.size_y = PW, PH, 1, 1, SIZE_Y
    f.resid_jobs = d_rjobs.ptr if mode != "jobs" else 0
    f.scale_table = d_arena.ptr + pitches[0] * PH + 2 * pitches[1] * (PH // 2) if mode == "resid_table" else 0
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    dev.vvc355_itx_frame_build(None, d_f.ptr, ctypes.addressof(f))
    dev.vvc355_stream_sync(None)

    want_j, want_r = expected(tus, f)
    for name, buf, want in (("jobs", d_jobs, want_j.view(np.uint8)), ("resid_jobs", d_rjobs, want_r.view(np.uint8))):
        got = buf.to_host(np.uint8, (len(want) + TAIL,))
        assert (got[len(want):] == 0xA5).all(), f"{name}: the 0xA5 tail was written"
        if name == "resid_jobs" and mode == "jobs":
            assert (got == 0xA5).all(), "resid_jobs written although the frame has none"
            continue
        bad = np.flatnonzero(got[:len(want)] != want)
        size = len(want) // n
        assert len(bad) == 0, f"{name}: {len(bad)} bytes differ, first in job {bad[0] // size} at byte {bad[0] % size}"
    assert (d_tus.to_host(np.uint8, (tus.nbytes + TAIL,))[tus.nbytes:] == 0xA5).all()
    if n >= 63:
        fl = tus["flags"]
        assert all(((fl & b) != 0).any() and ((fl & b) == 0).any() for b in (1, 2, 4, 8, 16, 32, 64)) and len(set(tus["c_idx"])) == 3

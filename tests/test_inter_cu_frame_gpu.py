"""GPU parity of the affine and geometric-partition stage drivers (vvc355_affine_frame_pass, vvc355_gpm_frame_pass): the job arrays the
builder kernels write from the decoder's tables and one record per coding unit, against the restatement of pred_affine_blk /
pred_gpm_blk in affine_gpm_cases.py (GPM weights addressed in the reference's own masks, tests/golden/gpm_tables.npz), then the
predicted picture against the oracle's block functions run on the expected jobs."""
import ctypes
import os

import numpy as np
import pytest

import affine_gpm_cases as agc
import bipred_cases as bc
from conftest import ROOT
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "gpm_tables.npz"))
BCW_W1 = {5, 3, 10, -2}


def assert_jobs_equal(got, exp, what, skip=()):
    for name in exp.dtype.names:
        if name in skip:
            continue
        bad = np.nonzero(np.any((got[name] != exp[name]).reshape(len(exp), -1), axis=1))[0]
        assert len(bad) == 0, f"{what}: field {name} differs in {len(bad)} jobs, first {bad[0]}: {got[name][bad[0]]} != {exp[name][bad[0]]}"


def tile_weights(read, addr, step_x, step_y, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return read(addr, ys * step_y + xs * step_x)


# (bd, (hs, vs, chroma), width, height, motion range); the last: motion far outside the picture (edge emulation)
CASES = [(10, (1, 1, True), 256, 192, 20 * 16), (8, (0, 0, True), 256, 192, 20 * 16), (12, (1, 0, True), 256, 192, 20 * 16),
         (10, (0, 0, False), 256, 192, 20 * 16), (10, (1, 1, True), 128, 128, 300 * 16)]


@pytest.mark.parametrize("bd,fmt,w,h,mv_range", CASES)
def test_affine_gpm_frame_pass(dev, orc, bd, fmt, w, h, mv_range):
    hs, vs, chroma = fmt
    rng = np.random.default_rng(0xAF6 + bd + 5 * hs + 3 * vs + 11 * chroma + w)
    isz = 1 if bd == 8 else 2
    n_comp = 3 if chroma else 1
    dims = [(w, h)] + [(w >> hs, h >> vs)] * 2
    work = agc.AffineGpmWork(rng, w, h, hs, vs, chroma, isz, mv_range=mv_range)
    base = [bc.smooth_picture(rng, ph, pw, bd) for (pw, ph) in dims]
    refs = [[[bc.shifted(base[c], (2 * l - 1) * (r + 1) >> (hs if c else 0), (1 - 2 * l) * (r + 2) >> (vs if c else 0)) for c in range(3)] for r in range(2)] for l in range(2)]
    lut = np.sort(np.random.default_rng(0x10C5 + bd).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)      # fc->ps.lmcs.fwd_lut
    sentinel = (1 << bd) // 3
    masks = np.ascontiguousarray(GOLDEN["ff_vvc_gpm_weights"])

    # ---- expected jobs on host memory, through the oracle
    want = [np.full((ph, pw), sentinel, base[0].dtype) for (pw, ph) in dims]
    h_jl, h_jc = work.expect_affine(lambda c: (want[c].ctypes.data, dims[c][0] * isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * isz),
                                    lambda u: work.aff.ctypes.data + u * agc.AFFINE_CU_DT.itemsize, lut.ctypes.data)
    h_g = work.expect_gpm(lambda c: (want[c].ctypes.data, dims[c][0] * isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * isz),
                          lut.ctypes.data, masks.ctypes.data, GOLDEN)
    agc.call(orc.orc_affine_block, bd, h_jl)
    agc.call(orc.orc_bipred_block, bd, h_jc)
    agc.call(orc.orc_gpm_block, bd, h_g)

    # ---- device
    pitches = [batch.plane_pitch(d[0], isz) for d in dims]
    d_dst = [batch.DeviceBuffer.from_host(batch.to_pitched(np.full((ph, pw), sentinel, base[0].dtype))) for (pw, ph) in dims]
    d_ref = [[[batch.DeviceBuffer.from_host(batch.to_pitched(refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
    t_refs = agc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], [[pitches] * 2] * 2)
    d_reft = batch.DeviceBuffer.from_host(np.frombuffer(bytes(t_refs), np.uint8))
    d_mvf = batch.DeviceBuffer.from_host(work.mvf.view(np.uint8))
    d_sl = batch.DeviceBuffer.from_host(np.frombuffer(bytes(work.slices), np.uint8))
    d_lut = batch.DeviceBuffer.from_host(lut)
    d_acu, d_gcu = batch.DeviceBuffer.from_host(work.aff.view(np.uint8)), batch.DeviceBuffer.from_host(work.gpm.view(np.uint8))
    d_jl = batch.DeviceBuffer(h_jl.nbytes)
    d_jc = batch.DeviceBuffer(h_jc.nbytes) if chroma else None
    d_g = batch.DeviceBuffer(h_g.nbytes)
    pic = work.pic([b.ptr for b in d_dst], pitches, d_mvf.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr)
    af = abi.AffineFrame(pic=pic, cus=d_acu.ptr, jobs_luma=d_jl.ptr, jobs_chroma=d_jc.ptr if chroma else 0, n_cus=len(work.aff), n_jobs=work.n_aff_jobs)
    gf = abi.GpmFrame(pic=pic, cus=d_gcu.ptr, jobs=d_g.ptr, n_cus=len(work.gpm), n_jobs=work.n_gpm_jobs)
    d_af, d_gf = (batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8)) for f in (af, gf))
    dev.vvc355_affine_frame_pass(None, bd, d_af.ptr, ctypes.addressof(af))
    dev.vvc355_gpm_frame_pass(None, bd, d_gf.ptr, ctypes.addressof(gf))
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0

    # ---- the job arrays: the same walk with the device addresses
    e_jl, e_jc = work.expect_affine(lambda c: (d_dst[c].ptr, pitches[c]), lambda l, r, c: (d_ref[l][r][c].ptr, pitches[c]),
                                    lambda u: d_acu.ptr + u * agc.AFFINE_CU_DT.itemsize, d_lut.ptr)
    assert_jobs_equal(d_jl.to_host(agc.AFFINE_JOB_DT, (work.n_aff_jobs,)), e_jl, "affine luma")
    if chroma:
        assert len(e_jc) == 2 * (work.n_aff_jobs >> (hs + vs))
        assert_jobs_equal(d_jc.to_host(agc.BIPRED_JOB_DT, (len(e_jc),)), e_jc, "affine chroma")
    e_g = work.expect_gpm(lambda c: (d_dst[c].ptr, pitches[c]), lambda l, r, c: (d_ref[l][r][c].ptr, pitches[c]), d_lut.ptr, 0, GOLDEN)
    g_g = d_g.to_host(agc.GPM_JOB_DT, (work.n_gpm_jobs,))
    assert_jobs_equal(g_g["base"], e_g["base"], "gpm")
    # GPM weights: the values the device jobs address in the library's masks against those the reference's addressing reads
    flat = masks.reshape(-1)
    for k in range(work.n_gpm_jobs):
        jw, jh = int(h_g["base"]["w"][k]), int(h_g["base"]["h"][k])
        exp = tile_weights(lambda a, idx: flat[a - masks.ctypes.data + idx], int(h_g["weights"][k]), int(h_g["step_x"][k]), int(h_g["step_y"][k]), jw, jh)
        sx, sy = int(g_g["step_x"][k]), int(g_g["step_y"][k])
        assert sx > 0 and sy > 0
        span = np.zeros((jh - 1) * sy + (jw - 1) * sx + 1, np.uint8)
        dev.vvc355_download(span.ctypes.data, int(g_g["weights"][k]), span.nbytes)
        got = tile_weights(lambda a, idx: span[idx], 0, sx, sy, jw, jh)
        assert np.array_equal(got, exp), f"gpm job {k}: weights differ"

    # ---- the picture
    for c in range(n_comp):
        got = d_dst[c].to_host(want[c].dtype, (dims[c][1], pitches[c] // isz))[:, :dims[c][0]]
        bad = np.argwhere(got != want[c])
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"
        sx, sy = (hs, vs) if c else (0, 0)
        outside = ~work.covered[::1 << sy, ::1 << sx]
        assert outside.any() and (want[c][outside] == sentinel).all()
        assert (want[c][~outside] != sentinel).mean() > 0.9                     # the units were predicted

    # ---- the case mix
    if w * h >= 256 * 192:
        used = [(e_jl["pred_flag"] & (1 << l)) != 0 for l in range(2)]
        assert set(np.unique(e_jl["pred_flag"])) == {1, 2, 3}
        for l, key in enumerate(("prof0", "prof1")):
            assert set(np.unique(e_jl[key][used[l]])) == {0, 1}
        bi = e_jl["pred_flag"] == 3
        assert (bi & (e_jl["weight_flag"] == 0)).any() and (~bi & (e_jl["weight_flag"] == 1)).any()
        assert (bi & (e_jl["denom"] == 2) & np.isin(e_jl["w1"], list(BCW_W1))).any()                # bcw weights
        assert (bi & (e_jl["weight_flag"] == 1) & (e_jl["denom"] == 6)).any()                         # explicit weights
        assert sorted(set(work.gpm["partition_idx"].tolist())) == list(range(64))
        angles = GOLDEN["ff_vvc_gpm_angle_idx"][work.gpm["partition_idx"]]
        assert set(GOLDEN["ff_vvc_gpm_angle_to_mirror"][angles].tolist()) == {0, 1, 2}
        assert ((h_g["step_x"] < 0).any() and (h_g["step_y"] < 0).any())
        assert {(int(cu["cb_width"]), int(cu["cb_height"])) for cu in work.aff} >= {(16, 16), (64, 64), (32, 16), (16, 64)}
        assert {(int(cu["cb_width"]), int(cu["cb_height"])) for cu in work.gpm} >= {(8, 8), (8, 32), (32, 8), (16, 64), (64, 64)}

"""GPU parity of the packed-level transform entries (vvc355_itx_shape_batch_lv, vvc355_itx_batch_lv) and of vvc355_levels_expand, bit-exact.
Each batch runs three ways: the oracle (orc_dequant + orc_itx, + orc_add_residual), the int32 entry on the int32 arena, and the packed entry
on the int16 group stream (levels_cases.py packs it) with an arena that holds no levels; all three must agree."""
import ctypes

import numpy as np
import pytest

import levels_cases as lc
import recon_cases
from conftest import P, rand_pixels
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu
DCT2 = 0


def _job_specs(rng, lw, lh, n, bd, int32_frac=0.0, wild_every=0):
    """Random transform blocks of one shape: types the table holds, windows, fused dequant with / without dep-quant, add or store."""
    w, h = 1 << lw, 1 << lh
    specs = []
    for i in range(n):
        trh = int(rng.integers(0, 3)) if 4 <= w <= 32 else DCT2
        trv = int(rng.integers(0, 3)) if 4 <= h <= 32 else DCT2
        if w == 1 or h == 1:
            trh = trv = DCT2
        lim_w, lim_h = lc.nz_limits(trh, trv, w, h)
        nzw, nzh = int(rng.integers(1, lim_w + 1)), int(rng.integers(1, lim_h + 1))
        if rng.random() < 0.1:
            trh = trv = DCT2
            nzw = nzh = 1                                     # DC-only shortcut
        rbits = 15
        c = lc.windowed_block(rng, w, h, nzw, nzh, bits=None if rng.random() < 0.7 else 15)
        fused = rng.random() < 0.6
        wild = wild_every and i % wild_every == int(rng.integers(0, wild_every)) % wild_every
        if fused and rng.random() < 0.2:
            c[0, 0] = int(rng.choice([32767, -32768, -32767]))  # extreme levels: the scaling process clips them to the range
        if wild:
            # range 20 with levels at the int16 extremes: not eligible for the 16-bit path, so the whole workgroup takes the generic arithmetic
            rbits, fused = 20, True
            c[:nzh, :nzw] = rng.choice([32767, -32768, -32767, 0], size=(nzh, nzw))
        spec = dict(lw=lw, lh=lh, trh=trh, trv=trv, nzw=nzw, nzh=nzh, c=c, range=rbits, fused=fused,
                    qp=int(rng.integers(0, 52)), dep=int(rng.integers(0, 2)), store=bool(rng.random() < 0.4),
                    int32=bool(rng.random() < int32_frac))
        specs.append(spec)
    return specs


def _run_three_ways(dev, orc, bd, specs, launch_int32, launch_packed):
    isz = 1 if bd == 8 else 2
    rng = np.random.default_rng(len(specs) * 7 + bd)
    n = len(specs)
    w, h = 1 << max(s["lw"] for s in specs), 1 << max(s["lh"] for s in specs)
    cols = max(1, 256 // w)
    rows = (n + cols - 1) // cols
    pic = rand_pixels(rng, (rows * h, cols * w), bd)
    want = pic.copy()
    want_res = []
    offs, off = [], 0
    for i, s in enumerate(specs):
        bw, bh = 1 << s["lw"], 1 << s["lh"]
        ref = s["c"].copy()
        if s["fused"]:
            orc.orc_dequant(P(ref), s["lw"], s["lh"], 0, 0, bw - 1, bh - 1, s["qp"], 0, s["dep"], bd, s["range"], None, 1, -1)
        assert orc.orc_itx(s["trh"], s["trv"], s["lw"], s["lh"], P(ref), s["nzw"], s["nzh"], s["range"], bd) == 0
        x0, y0 = (i % cols) * w, (i // cols) * h
        if s["store"]:
            want_res.append(ref)
        else:
            blk = np.ascontiguousarray(want[y0:y0 + bh, x0:x0 + bw])
            orc.orc_add_residual(bd, P(blk), P(ref), bw, bh, bw * isz)
            want[y0:y0 + bh, x0:x0 + bw] = blk
            want_res.append(None)
        offs.append(off)
        off += bw * bh
    levels, lv = lc.pack_all([s["c"] for s in specs], force_int32={i for i, s in enumerate(specs) if s["int32"]})
    assert (lv["flags"] == 0).sum() >= n // 2

    results = []
    for mode in ("int32", "packed"):
        pitched = batch.to_pitched(pic)
        pitch = pitched.shape[1] * isz
        d_pic = batch.DeviceBuffer.from_host(pitched)
        arena = np.full(off, 0x7EADBEEF, np.int32)             # the packed run's arena holds no levels, except for the int32 blocks
        for i, s in enumerate(specs):
            if mode == "int32" or lv[i]["flags"]:
                arena[offs[i]:offs[i] + s["c"].size] = s["c"].ravel()
        d_arena = batch.DeviceBuffer.from_host(arena)
        arr = (abi.ItxJob * n)()
        for i, s in enumerate(specs):
            j = arr[i]
            x0, y0 = (i % cols) * w, (i // cols) * h
            j.coeffs = d_arena.ptr + offs[i] * 4
            j.dst, j.dst_stride, j.store_coeffs = (0, 0, 1) if s["store"] else (d_pic.ptr + y0 * pitch + x0 * isz, pitch, 0)
            j.trh, j.trv, j.log2_w, j.log2_h, j.nzw, j.nzh, j.range, j.bd = s["trh"], s["trv"], s["lw"], s["lh"], s["nzw"], s["nzh"], s["range"], bd
            if s["fused"]:
                j.dq_flags, j.dq_qp, j.log2_matrix_size, j.dc = 1 | (s["dep"] << 1), s["qp"], 1, -1
        d_jobs = batch.jobs_to_device(arr)
        if mode == "int32":
            launch_int32(d_jobs.ptr, n)
        else:
            d_lv = batch.DeviceBuffer.from_host(lv.view(np.uint8))
            d_levels = batch.DeviceBuffer.from_host(levels)
            assert d_levels.ptr % 32 == 0
            launch_packed(d_jobs.ptr, d_lv.ptr, d_levels.ptr, n)
        dev.vvc355_stream_sync(None)
        got_pic = d_pic.to_host(pitched.dtype, pitched.shape)[:, :pic.shape[1]]
        got_arena = d_arena.to_host(np.int32, arena.shape)
        results.append((got_pic, got_arena))
        bad = np.argwhere(got_pic != want)
        assert len(bad) == 0, f"{mode}: {len(bad)} samples differ, first at {bad[0].tolist()} (block {bad[0][0] // h * cols + bad[0][1] // w})"
        for i, s in enumerate(specs):
            if s["store"]:
                assert np.array_equal(got_arena[offs[i]:offs[i] + s["c"].size].reshape(s["c"].shape), want_res[i]), (mode, i, s["lw"], s["lh"])
    assert np.any(want != pic)
    return results


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_shape_batch_lv_every_shape(dev, orc, bd):
    rng = np.random.default_rng(0x5EED1E10 + bd)
    for lw in range(2, 7):
        for lh in range(2, 7):
            specs = _job_specs(rng, lw, lh, 48, bd)
            _run_three_ways(dev, orc, bd, specs,
                            lambda jp, n: dev.vvc355_itx_shape_batch(None, bd, jp, n, lw, lh),
                            lambda jp, lp, sp, n: dev.vvc355_itx_shape_batch_lv(None, bd, jp, lp, sp, n, lw, lh))


def test_shape_batch_lv_mixed_and_fallback(dev, orc):
    """Packed and VVC355_LEVELS_INT32 jobs in one launch; one job per workgroup that sends the workgroup to the generic arithmetic."""
    rng = np.random.default_rng(0x5EED1E20)
    for (lw, lh) in ((2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (3, 5), (5, 3), (2, 6), (6, 2), (4, 6)):
        tbs = max(1, 256 // ((1 << (lw + lh)) // 16))
        for kind in ("mixed", "wild"):
            specs = _job_specs(rng, lw, lh, max(64, 3 * tbs), 10, int32_frac=0.3 if kind == "mixed" else 0.0,
                               wild_every=tbs if kind == "wild" else 0)
            _run_three_ways(dev, orc, 10, specs,
                            lambda jp, n: dev.vvc355_itx_shape_batch(None, 10, jp, n, lw, lh),
                            lambda jp, lp, sp, n: dev.vvc355_itx_shape_batch_lv(None, 10, jp, lp, sp, n, lw, lh))


@pytest.mark.parametrize("bd", [8, 12])
def test_itx_batch_lv_small_sizes_and_buckets(dev, orc, bd):
    """The generic entry: blocks below 4 (1x16, 16x1, 2xN, Nx2) and every max_log2_area bucket, packed and int32 mixed."""
    rng = np.random.default_rng(0x5EED1E30 + bd)
    shapes = [(0, 4), (4, 0), (0, 5), (5, 0), (6, 0), (1, 2), (1, 3), (1, 4), (1, 5), (2, 1), (3, 1), (4, 1), (5, 1),
              (2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (3, 5), (5, 5), (4, 6), (6, 6)]
    for (lw, lh) in shapes:
        area = lw + lh
        specs = _job_specs(rng, lw, lh, 40, bd, int32_frac=0.2)
        for s in specs:
            if s["lw"] < 2 or s["lh"] < 2:
                s["fused"] = False          # the fused scaling of the generic loader assumes 4-wide rows; these blocks are scaled beforehand
        _run_three_ways(dev, orc, bd, specs,
                        lambda jp, n: dev.vvc355_itx_batch(None, bd, jp, n, area),
                        lambda jp, lp, sp, n: dev.vvc355_itx_batch_lv(None, bd, jp, lp, sp, n, area))


def test_levels_expand_then_lfnst(dev, orc):
    """vvc355_levels_expand writes each packed job's window and nothing else; LFNST blocks then go lfnst_batch -> itx on int32."""
    orc.orc_ilfnst_transform.restype = ctypes.c_int
    orc.orc_ilfnst_transform.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
    rng = np.random.default_rng(0x5EED1E40)
    SENT = 0x7EADBEEF
    # (lw, lh, kind): ts = full-block window (transform skip / BDPCM), lfnst = window of the transform after LFNST, other = a level window
    cases = [(lw, lh, "ts") for lw in range(1, 6) for lh in range(1, 6)] + [(0, 4, "ts"), (4, 0, "ts")]
    cases += [(lw, lh, "lfnst") for (lw, lh) in ((2, 2), (3, 3), (2, 4), (4, 2), (3, 4), (4, 4), (5, 3), (6, 6), (2, 3), (3, 2))]
    cases += [(int(rng.integers(0, 7)), int(rng.integers(0, 7)), "other") for _ in range(60)]
    cases = [c for c in cases if (1 << c[0]) * (1 << c[1]) >= 4] * 3
    blocks, jobs_win, offs, off = [], [], [], 0
    for (lw, lh, kind) in cases:
        w, h = 1 << lw, 1 << lh
        if kind == "ts":
            nzw, nzh = w, h
            c = lc.windowed_block(rng, w, h, w, h, bits=15 if rng.random() < 0.5 else None)
        elif kind == "lfnst":
            nzw = nzh = 8 if (w >= 8 and h >= 8) else 4
            c = np.zeros((h, w), np.int32)
            c[:min(h, 4), :min(w, 4)] = rng.integers(-40, 41, size=(min(h, 4), min(w, 4)))
        else:
            nzw, nzh = int(rng.integers(1, min(w, 32) + 1)), int(rng.integers(1, min(h, 32) + 1))
            c = lc.windowed_block(rng, w, h, nzw, nzh)
        blocks.append(c); jobs_win.append((lw, lh, nzw, nzh, kind))
        off += 64                                            # a gap of sentinels between blocks
        offs.append(off); off += w * h
    off += 64
    force = {i for i in range(len(blocks)) if i % 9 == 4}  # some int32 blocks: expand leaves them alone
    levels, lv = lc.pack_all(blocks, force_int32=force)
    arena = np.full(off, SENT, np.int32)
    d_arena = batch.DeviceBuffer.from_host(arena)
    arr = (abi.ItxJob * len(blocks))()
    for i, (lw, lh, nzw, nzh, kind) in enumerate(jobs_win):
        arr[i].coeffs, arr[i].log2_w, arr[i].log2_h, arr[i].nzw, arr[i].nzh = d_arena.ptr + offs[i] * 4, lw, lh, nzw, nzh
        arr[i].range, arr[i].bd, arr[i].store_coeffs = 15, 10, 1
    d_jobs = batch.jobs_to_device(arr)
    d_lv, d_levels = batch.DeviceBuffer.from_host(lv.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
    dev.vvc355_levels_expand(None, d_jobs.ptr, d_lv.ptr, d_levels.ptr, len(blocks))
    dev.vvc355_stream_sync(None)
    got = d_arena.to_host(np.int32, arena.shape)
    expect = arena.copy()
    for i, (lw, lh, nzw, nzh, kind) in enumerate(jobs_win):
        w, h = 1 << lw, 1 << lh
        if i in force:
            continue
        full = lc.unpack(int(lv[i]["groups"]), levels, int(lv[i]["first"]), w, h)
        assert np.array_equal(full, blocks[i])
        blk = expect[offs[i]:offs[i] + w * h].reshape(h, w)
        blk[:nzh, :nzw] = full[:nzh, :nzw]
    bad = np.flatnonzero(got != expect)
    assert len(bad) == 0, f"{len(bad)} arena words differ, first at {bad[0]}"

    # LFNST blocks: expand -> lfnst_batch (scaling + ilfnst_transform) -> itx on the int32 arena, against the oracle
    idx = [i for i, jw in enumerate(jobs_win) if jw[4] == "lfnst" and i not in force]
    lj = (abi.LfnstJob * len(idx))()
    xj = (abi.ItxJob * len(idx))()
    want = []
    for k, i in enumerate(idx):
        lw, lh, nzw, nzh, _ = jobs_win[i]
        w, h = 1 << lw, 1 << lh
        mode, lidx, qp, dep = int(rng.integers(-14, 81)), int(rng.integers(1, 3)), int(rng.integers(20, 40)), int(rng.integers(0, 2))
        e = blocks[i].copy()
        orc.orc_dequant(P(e), lw, lh, 0, 0, min(w, 4) - 1, min(h, 4) - 1, qp, 0, dep, 10, 15, None, 1, -1)
        orc.orc_ilfnst_transform(P(e), w, h, mode, lidx, 15)
        assert orc.orc_itx(DCT2, DCT2, lw, lh, P(e), nzw, nzh, 15, 10) == 0
        want.append(e)
        j = lj[k]
        j.coeffs, j.log2_w, j.log2_h, j.max_x, j.max_y = d_arena.ptr + offs[i] * 4, lw, lh, min(w, 4) - 1, min(h, 4) - 1
        j.qp, j.dequant, j.dep_quant, j.bit_depth, j.range, j.log2_matrix_size, j.dc = qp, 1, dep, 10, 15, 1, -1
        j.pred_mode_intra, j.lfnst_idx = mode, lidx
        xj[k] = arr[i]
    d_lj, d_xj = batch.jobs_to_device(lj), batch.jobs_to_device(xj)
    dev.vvc355_lfnst_batch(None, d_lj.ptr, len(idx))
    # the transform after LFNST reads only its window (what expand wrote); its residual covers the whole block
    dev.vvc355_itx_batch(None, 10, d_xj.ptr, len(idx), 12)
    dev.vvc355_stream_sync(None)
    got = d_arena.to_host(np.int32, arena.shape)
    for k, i in enumerate(idx):
        lw, lh = jobs_win[i][:2]
        assert np.array_equal(got[offs[i]:offs[i] + (1 << (lw + lh))].reshape(1 << lh, 1 << lw), want[k]), (lw, lh)


@pytest.mark.parametrize("bd", [10, 8])
def test_frame_build_then_packed_batches(dev, orc, bd):
    """Records -> vvc355_itx_frame_build -> packed shape batches (jobs and side records offset alike) -> chroma residual scaling: the planes
    equal those of the same records run through the int32 arena."""
    rng = np.random.default_rng(0x5EED1E50 + bd)
    isz = 1 if bd == 8 else 2
    pw, ph = 256, 128
    dims = [(pw, ph), (pw // 2, ph // 2), (pw // 2, ph // 2)]
    planes = [rand_pixels(rng, (d[1], d[0]), bd) for d in dims]
    model = recon_cases.ReconWork.lmcs_model(rng, bd)
    recs, coeff_off = [], 0
    for y in range(0, ph, 16):
        for x in range(0, pw, 16):
            for c in (1, 2):
                recs.append((c, x // 2, y // 2, 3, 3, coeff_off)); coeff_off += 64
            recs.append((0, x, y, 4, 4, coeff_off)); coeff_off += 256
    recs.sort(key=lambda r: r[3])                           # binned by shape: 8x8 chroma first, then 16x16 luma
    n = len(recs)
    tus = np.zeros(n, np.dtype(abi.ItxTu, align=True))
    blocks = []
    for i, (c, x, y, lw, lh, off) in enumerate(recs):
        t = tus[i]
        t["coeff_off"], t["x0"], t["y0"], t["log2_w"], t["log2_h"], t["c_idx"] = off, x, y, lw, lh, c
        t["nzw"], t["nzh"] = int(rng.integers(1, (1 << lw) + 1)), int(rng.integers(1, (1 << lh) + 1))
        t["qp"], t["tr"] = int(rng.integers(22, 40)), int(rng.integers(0, 3)) | int(rng.integers(0, 3)) << 4
        flags = 1 | (int(rng.integers(0, 2)) << 1)
        if c and rng.random() < 0.7:
            flags |= 4 | 64 | ((((2 * x) & ~63) > 0) << 4) | ((((2 * y) & ~63) > 0) << 5)
        t["flags"] = flags
        blocks.append(lc.windowed_block(rng, 1 << lw, 1 << lh, int(t["nzw"]), int(t["nzh"])))
    force = {i for i in range(n) if rng.random() < 0.1}
    levels, lv = lc.pack_all(blocks, force_int32=force)
    n8 = sum(1 for r in recs if r[3] == 3)
    jsz, lsz = ctypes.sizeof(abi.ItxJob), lv.dtype.itemsize
    outs = []
    for mode in ("int32", "packed"):
        arena = np.zeros(coeff_off, np.int32)
        for i, r in enumerate(recs):
            if mode == "int32" or i in force:
                arena[r[5]:r[5] + blocks[i].size] = blocks[i].ravel()
        pitched = [batch.to_pitched(p) for p in planes]
        d_planes = [batch.DeviceBuffer.from_host(p) for p in pitched]
        d_arena, d_tus = batch.DeviceBuffer.from_host(arena), batch.DeviceBuffer.from_host(tus.view(np.uint8))
        d_jobs = batch.DeviceBuffer.from_host(np.zeros(n * jsz, np.uint8))
        d_rjobs = batch.DeviceBuffer.from_host(np.zeros(n * ctypes.sizeof(abi.LmcsResidJob), np.uint8))
        d_model = batch.DeviceBuffer.from_host(np.frombuffer(bytes(model), np.uint8))
        f = abi.ItxFrame()
        f.tus, f.jobs, f.coeffs, f.n_tus = d_tus.ptr, d_jobs.ptr, d_arena.ptr, n
        for c in range(3):
            f.plane[c], f.stride[c] = d_planes[c].ptr, pitched[c].shape[1] * isz
        f.range, f.bd, f.pixel_shift = 15, bd, int(isz == 2)
        f.width, f.height, f.hs, f.vs, f.size_y = pw, ph, 1, 1, 64
        f.resid_jobs, f.scale_table = d_rjobs.ptr, 0
        d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
        dev.vvc355_itx_frame_build(None, d_f.ptr, ctypes.addressof(f))
        if mode == "int32":
            dev.vvc355_itx_shape_batch(None, bd, d_jobs.ptr, n8, 3, 3)
            dev.vvc355_itx_shape_batch(None, bd, d_jobs.ptr + n8 * jsz, n - n8, 4, 4)
        else:
            d_lv, d_levels = batch.DeviceBuffer.from_host(lv.view(np.uint8)), batch.DeviceBuffer.from_host(levels)
            dev.vvc355_itx_shape_batch_lv(None, bd, d_jobs.ptr, d_lv.ptr, d_levels.ptr, n8, 3, 3)
            dev.vvc355_itx_shape_batch_lv(None, bd, d_jobs.ptr + n8 * jsz, d_lv.ptr + n8 * lsz, d_levels.ptr, n - n8, 4, 4)
        dev.vvc355_lmcs_chroma_resid_batch(None, bd, d_rjobs.ptr, n, d_model.ptr)
        dev.vvc355_stream_sync(None)
        outs.append([d_planes[c].to_host(pitched[c].dtype, pitched[c].shape)[:, :dims[c][0]] for c in range(3)])
    for c in range(3):
        bad = np.argwhere(outs[0][c] != outs[1][c])
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at {bad[0].tolist()}"
        assert np.any(outs[1][c] != planes[c])

"""CPU: properties of the oracle that hold independently of both implementations (for the callers and context-taking slots, which
are not pinned against the reference, these are the strongest checks available; the leaf slots are pinned by test_oracle_ref_cpu.py):
transform-matrix identities, DC gains on flat input, identity cases, mode-helper tables."""
import ctypes

import numpy as np
import pytest

from conftest import P, px_dtype, rand_pixels


def table(orc, name, ctype, shape):
    n = int(np.prod(shape))
    return np.ctypeslib.as_array((ctype * n).in_dll(orc, "orc_tab_" + name)).reshape(shape).astype(np.int64)


def inv_matrix(orc, ttype, n, nz=None):
    """Matrix M with out = M @ in realised by orc_inv_tx_1d (column k = response to unit input k)."""
    orc.orc_inv_tx_1d.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_size_t]
    m = np.zeros((n, n), np.int64)
    for k in range(n):
        v = np.zeros(n, np.int32)
        v[k] = 1
        orc.orc_inv_tx_1d(ttype, n, P(v), 1, n if nz is None else nz)
        m[:, k] = v
    return m


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_dct2_matrix_is_near_orthogonal_and_nested(orc, n):
    m = inv_matrix(orc, 0, n)
    gram = m.T @ m                       # basis functions are the columns' duals: M = T^T, T T^T ~ 64^2 * n * I
    diag = np.diag(gram)
    assert np.all(np.abs(diag - 64 * 64 * n) <= 64 * 64 * n * 0.01)
    off = gram - np.diag(diag)
    assert np.max(np.abs(off)) <= 64 * 64 * n * 0.01
    assert np.all(m[:, 0] == 64)         # DC basis
    if n >= 4:                           # even basis functions of size n are the size n/2 basis, mirrored
        half = inv_matrix(orc, 0, n // 2)
        assert np.array_equal(m[: n // 2, 0::2], half)
        assert np.array_equal(m[n // 2:, 0::2][::-1], half)


def test_dct2_64_reads_only_32_inputs_and_gates_by_nz(orc):
    m = inv_matrix(orc, 0, 64)
    assert np.all(m[:, 32:] == 0) and np.all(m[:, :32] != 0)
    gram = m[:, :32].T @ m[:, :32]
    assert np.max(np.abs(gram - np.diag(np.diag(gram)))) <= 64 * 64 * 64 * 0.01
    # nz gating: input k contributes iff k < 2 or nz > 2^floor(log2 k) (vvc_itx_1d.c:64-67)
    for nz in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32):
        g = inv_matrix(orc, 0, 32, nz)
        used = [k for k in range(32) if np.any(g[:, k])]
        want = [k for k in range(32) if k < 2 or nz > (1 << int(np.log2(k)))]
        assert used == want, (nz, used)


@pytest.mark.parametrize("n", [4, 8, 16, 32])
def test_dst7_dct8_tables(orc, n):
    dst7 = table(orc, f"dst7_{n}", ctypes.c_int8, (n, n))
    dct8 = table(orc, f"dct8_{n}", ctypes.c_int8, (n, n))
    # closed forms of the real-valued transforms, scaled like the standard's integer matrices
    k, j = np.mgrid[0:n, 0:n]
    s7 = np.sqrt(4.0 / (2 * n + 1)) * np.sin(np.pi * (2 * k + 1) * (j + 1) / (2 * n + 1)) * 64 * np.sqrt(n)
    c8 = np.sqrt(4.0 / (2 * n + 1)) * np.cos(np.pi * (2 * k + 1) * (2 * j + 1) / (4 * n + 2)) * 64 * np.sqrt(n)
    assert np.max(np.abs(dst7 - s7)) <= 1.5
    assert np.max(np.abs(dct8 - c8)) <= 1.5
    assert np.array_equal(dct8, ((-1) ** k) * dst7[:, ::-1])
    g = dst7 @ dst7.T
    assert np.max(np.abs(g - np.diag(np.diag(g)))) <= 64 * 64 * n * 0.02


def test_itx_dc_response_and_zero(orc):
    orc.orc_itx.restype = ctypes.c_int
    for lw in range(1, 7):
        for lh in range(1, 7):
            w, h = 1 << lw, 1 << lh
            c = np.zeros((h, w), np.int32)
            assert orc.orc_itx(0, 0, lw, lh, P(c), 1, 1, 15, 10) == 0 and not c.any()
            c[0, 0] = 1 << 12
            assert orc.orc_itx(0, 0, lw, lh, P(c), 1, 1, 15, 10) == 0
            # a DC coefficient reconstructs to a flat block: 64*64*c / 2^(7 + 5 + 15 - 10)
            assert np.all(c == c[0, 0]) and abs(int(c[0, 0]) - (64 * 64 * (1 << 12) >> 17)) <= 1
    assert orc.orc_itx(1, 0, 1, 1, P(np.zeros(4, np.int32)), 1, 1, 15, 10) == -1     # DST7 has no 2-point form


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_interpolation_filters_have_unit_dc_gain(orc, bd):
    luma = table(orc, "inter_luma_filters", ctypes.c_int8, (3, 16, 8))
    chroma = table(orc, "inter_chroma_filters", ctypes.c_int8, (3, 32, 4))
    assert np.all(luma.sum(axis=2) == 64) and np.all(chroma.sum(axis=2) == 64)
    fl = table(orc, "intra_luma_filter", ctypes.c_int8, (2, 32, 4))
    assert np.all(fl.sum(axis=2) == 64)
    # flat picture in -> the same flat value out of put_uni for every fraction
    val = (1 << bd) * 3 // 5
    plane = np.full((48, 64), val, px_dtype(bd))
    ps = plane.itemsize
    for chroma_flag, tab in ((0, luma), (1, chroma)):
        for ph in (1, tab.shape[1] // 2, tab.shape[1] - 1):
            f = np.ascontiguousarray(tab[0, ph].astype(np.int8))
            for vfrac in (0, 1):
                for hfrac in (0, 1):
                    dst = np.zeros((16, 16), plane.dtype)
                    orc.orc_put_uni(bd, chroma_flag, vfrac, hfrac, P(dst), 16 * ps, P(plane, 8 * 64 + 8), 64 * ps, 16, P(f), P(f), 16)
                    assert np.all(dst == val)
                    d16 = np.zeros((16, 128), np.int16)
                    orc.orc_put(bd, chroma_flag, vfrac, hfrac, P(d16), P(plane, 8 * 64 + 8), 64 * ps, 16, P(f), P(f), 16)
                    assert np.all(d16[:, :16] == val << (14 - bd))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_filters_leave_flat_pictures_flat(orc, bd):
    rng = np.random.default_rng(bd)
    val = (1 << bd) // 3
    src = np.full((160, 176), val, px_dtype(bd))
    ps = src.itemsize
    off = 8 * 176 + 8
    # ALF: every tap difference is zero, whatever the coefficients
    coeff = rng.integers(-128, 128, size=(1024, 12)).astype(np.int16)
    clip = np.full((1024, 12), 1 << bd, np.int16)
    dst = np.zeros((128, 128), src.dtype)
    orc.orc_alf_filter_luma(bd, P(dst), 128 * ps, P(src, off), 176 * ps, 128, 128, P(coeff), P(clip), 124)
    assert np.all(dst == val)
    # classification of a flat block: no activity, no direction
    cls = np.full(1024, -1, np.int32); tr = np.full(1024, -1, np.int32)
    grad = np.zeros(66 * 66 * 4, np.int32)
    orc.orc_alf_classify(bd, P(cls), P(tr), P(src, off), 176 * ps, 128, 128, 124, P(grad))
    assert np.all(cls == 0) and np.all(tr == 3)
    # SAO edge: all neighbours equal -> category 0 offset (index 0 of the table)
    offs = np.array([5, 1, 2, 3, 4], np.int16)
    ess = 320 // ps                                   # implicit source stride of 320 bytes
    edge_src = np.full((40, ess), val, src.dtype)
    d = np.zeros((32, 32), src.dtype)
    orc.orc_sao_edge_filter(bd, P(d), P(edge_src, 2 * ess + 8), 32 * ps, P(offs), 2, 32, 32)
    assert np.all(d == val + 5)
    # deblocking a flat edge changes nothing
    img = np.full((24, 24), val, src.dtype)
    beta = np.array([40, 40, 0, 0], np.int32); tc = np.array([20, 20, 0, 0], np.int32)
    z = np.zeros(4, np.uint8); l7 = np.full(4, 7, np.uint8)
    orc.orc_lf_filter_luma(bd, 1, P(img, 8 * 24 + 12), 24 * ps, P(beta), P(tc), P(z), P(z), P(l7), P(l7), 0)
    assert np.all(img == val)
    # planar / DC prediction from flat references
    top = np.full(300, val, src.dtype); left = np.full(300, val, src.dtype)
    for name in ("orc_pred_planar", "orc_pred_dc"):
        blk = np.zeros((16, 32), src.dtype)
        getattr(orc, name)(bd, P(blk), P(top, 100), P(left, 100), 32, 16, 32)
        assert np.all(blk == val)


def test_intra_mode_helpers(orc):
    orc.orc_intra_pred_angle.restype = ctypes.c_int
    orc.orc_intra_inv_angle.restype = ctypes.c_int
    angles = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512]
    assert orc.orc_intra_pred_angle(50) == 0 and orc.orc_intra_pred_angle(18) == 0
    assert orc.orc_intra_pred_angle(66) == 32 and orc.orc_intra_pred_angle(2) == 32 and orc.orc_intra_pred_angle(34) == -32
    assert orc.orc_intra_pred_angle(80) == 512 and orc.orc_intra_pred_angle(-14) == 512
    for a in angles[1:]:
        for s in (1, -1):
            # the reference computes ROUND((float)(32 * 512.0 / angle)) (vvc_intra.c:683-690)
            f = np.float32(16384.0 / (s * a))
            want = int(-(-float(f) + 0.5)) if f < 0 else int(float(f) + 0.5)
            assert orc.orc_intra_inv_angle(s * a) == want, a


@pytest.mark.parametrize("bd", [8, 10])
def test_avg_of_equal_predictions_is_identity(orc, bd):
    rng = np.random.default_rng(3)
    px = rand_pixels(rng, (8, 128), bd)
    s = (px.astype(np.int32) << (14 - bd)).astype(np.int16)
    d = np.zeros((8, 16), px.dtype)
    orc.orc_avg(bd, P(d), 16 * d.itemsize, P(s), P(s), 16, 8)
    assert np.array_equal(d, px[:, :16])


def test_dequant_closed_form(orc):
    """8.7.3 with the flat matrix (m = 16) and levelScale[0][4] = 64: coeff * 64 * 16 * 2^(qp/6) >> bdShift.  For a square
    8x8 block at 10-bit, range 15, no dependent quantisation, bdShift = 10 + 0 + 3 + 10 - 15 = 8, so qp = 4 + 6k is an
    exact left shift by 2 + k (then the clip to 16 bits); transform skip uses bdShift = 10, i.e. a left shift by k."""
    rng = np.random.default_rng(5)
    c = rng.integers(-2000, 2000, size=(8, 8)).astype(np.int32)
    for k in range(4):
        a = c.copy()
        orc.orc_dequant(P(a), 3, 3, 0, 0, 7, 7, 4 + 6 * k, 0, 0, 10, 15, None, 1, -1)
        assert np.array_equal(a, np.clip(c << (2 + k), -(1 << 15), (1 << 15) - 1))
        b = c.copy()
        orc.orc_dequant(P(b), 3, 3, 0, 0, 7, 7, 4 + 6 * k, 1, 0, 10, 15, None, 1, -1)
        assert np.array_equal(b, np.clip(c << k, -(1 << 15), (1 << 15) - 1))
    # outside the scan rectangle nothing changes
    a = c.copy()
    orc.orc_dequant(P(a), 3, 3, 1, 2, 4, 5, 28, 0, 0, 10, 15, None, 1, -1)
    keep = np.ones((8, 8), bool); keep[2:6, 1:5] = False
    assert np.array_equal(a[keep], c[keep]) and np.any(a[~keep] != c[~keep])


@pytest.mark.parametrize("bd", [8, 10])
def test_bipred_integer_motion_reads_clamped_samples(orc, bd):
    """With whole-sample motion, no refinement and equal references, avg(put, put) gives back the reference samples; far
    outside the picture that must be the replicated border (edge emulation, vvc_inter.c:33-110)."""
    import ctypes
    import bipred_cases as bc
    from ffvvc_amd import abi
    bc.bind_oracle(orc)
    rng = np.random.default_rng(11)
    pw, ph = 64, 48
    ref = rand_pixels(rng, (ph, pw), bd)
    for (x, y, mvx, mvy) in [(16, 16, 0, 0), (0, 0, -5 * 16, -3 * 16), (48, 32, 9 * 16, 40 * 16), (32, 0, -100 * 16, 7 * 16)]:
        dst = np.zeros((16, 16), ref.dtype)
        j = abi.BipredJob()
        j.dst, j.ref0, j.ref1 = P(dst), P(ref), P(ref)
        j.dst_stride, j.ref0_stride, j.ref1_stride = 16 * ref.itemsize, pw * ref.itemsize, pw * ref.itemsize
        for k, v in enumerate((mvx, mvy, mvx, mvy)):
            j.mv[k] = v
        j.x, j.y, j.w, j.h, j.pic_w, j.pic_h = x, y, 16, 16, pw, ph
        orc.orc_bipred_block(bd, ctypes.byref(j))
        yy = np.clip(np.arange(16) + y + mvy // 16, 0, ph - 1)
        xx = np.clip(np.arange(16) + x + mvx // 16, 0, pw - 1)
        assert np.array_equal(dst, ref[yy][:, xx])


def test_bipred_dmvr_early_termination(orc):
    """Identical references with mirrored motion: the centre SAD is 0 < w*h, so there is no search, the motion stays and
    the sub-block BDOF flag is cleared (vvc_inter.c:712, :744-746)."""
    import ctypes
    import bipred_cases as bc
    from ffvvc_amd import abi
    bc.bind_oracle(orc)
    rng = np.random.default_rng(12)
    ref = bc.smooth_picture(rng, 64, 64, 10)
    dst = np.zeros((16, 16), ref.dtype)
    rec = abi.BipredResult()
    j = abi.BipredJob()
    j.dst, j.ref0, j.ref1, j.rec = P(dst), P(ref), P(ref), ctypes.addressof(rec)
    j.dst_stride, j.ref0_stride, j.ref1_stride = 32, 128, 128
    for k, v in enumerate((37, -21, 37, -21)):
        j.mv[k] = v
    j.x, j.y, j.w, j.h, j.pic_w, j.pic_h, j.dmvr, j.bdof = 24, 24, 16, 16, 64, 64, 1, 1
    orc.orc_bipred_block(10, ctypes.byref(j))
    assert list(rec.mv) == [37, -21, 37, -21] and rec.searched == 0 and rec.bdof == 0 and rec.min_sad == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_affine_without_refinement_is_plain_prediction(orc, bd):
    """PROF with all-zero diff_mv adds nothing: the refined sub-block equals the unrefined one (uni and bi), and whole-sample
    motion without weights gives back the (clamped) reference samples."""
    import ctypes
    from ffvvc_amd import abi
    orc.orc_affine_block.argtypes = [ctypes.c_int, ctypes.POINTER(abi.AffineJob)]
    orc.orc_affine_block.restype = None
    rng = np.random.default_rng(21)
    pw, ph = 48, 40
    ref = [rand_pixels(rng, (ph, pw), bd), rand_pixels(rng, (ph, pw), bd)]
    zeros = np.zeros((2, 2, 16), np.int16)
    for (x, y, mv, pf) in [(8, 8, (37, -21, -100, 55), 3), (0, 0, (-77, -13, 0, 0), 1), (44, 36, (0, 0, 250, 199), 2), (16, 4, (5, 9, 5, 9), 3)]:
        outs = []
        for prof in (0, 1):
            dst = np.zeros((4, 4), ref[0].dtype)
            j = abi.AffineJob()
            j.dst, j.ref0, j.ref1, j.diff_mv = P(dst), P(ref[0]), P(ref[1]), P(zeros)
            j.dst_stride, j.ref0_stride, j.ref1_stride = 4 * dst.itemsize, pw * dst.itemsize, pw * dst.itemsize
            for k in range(4):
                j.mv[k] = mv[k]
            j.x, j.y, j.pic_w, j.pic_h, j.pred_flag, j.prof0, j.prof1 = x, y, pw, ph, pf, prof, prof
            orc.orc_affine_block(bd, ctypes.byref(j))
            outs.append(dst)
        assert np.array_equal(outs[0], outs[1])
    dst = np.zeros((4, 4), ref[0].dtype)
    j = abi.AffineJob()
    j.dst, j.ref0, j.ref1, j.diff_mv = P(dst), P(ref[0]), P(ref[1]), P(zeros)
    j.dst_stride, j.ref0_stride, j.ref1_stride = 4 * dst.itemsize, pw * dst.itemsize, pw * dst.itemsize
    j.mv[0], j.mv[1] = -20 * 16, 3 * 16
    j.x, j.y, j.pic_w, j.pic_h, j.pred_flag = 4, 8, pw, ph, 1
    orc.orc_affine_block(bd, ctypes.byref(j))
    yy, xx = np.clip(np.arange(4) + 8 + 3, 0, ph - 1), np.clip(np.arange(4) + 4 - 20, 0, pw - 1)
    assert np.array_equal(dst, ref[0][yy][:, xx])


@pytest.mark.parametrize("bd", [8, 10])
def test_alf_frame_pass_matches_slot_chain_on_one_ctb(orc, bd):
    """orc_alf_frame_pass (ff_vvc_alf_filter restated, vvc_filter.c:1254-1318) on a one-CTB picture equals the slot functions
    chained by hand on an edge-replicated copy (all four edges[] set); a CTB with every flag off passes through."""
    from ffvvc_amd import abi
    orc.orc_alf_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.AlfFrame)]
    orc.orc_alf_frame_pass.restype = None
    rng = np.random.default_rng(0xA1F + bd)
    w, h, isz = 64, 48, (1 if bd == 8 else 2)
    dims = [(w, h), (w // 2, h // 2), (w // 2, h // 2)]
    src = [rand_pixels(rng, (d[1], d[0]), bd) for d in dims]
    coeff = rng.integers(-40, 40, size=(25, 12)).astype(np.int16)
    clipi = rng.integers(0, 4, size=(25, 12)).astype(np.uint8)
    ccoef = rng.integers(-48, 48, size=(8, 6)).astype(np.int16)
    cclip = rng.integers(0, 4, size=(8, 6)).astype(np.uint8)
    cc = rng.integers(-32, 32, size=(4, 7)).astype(np.int16)
    sl = abi.AlfSlice()
    sl.luma_coeff[1], sl.luma_clip_idx[1] = P(coeff), P(clipi)
    sl.chroma_coeff, sl.chroma_clip_idx, sl.cc_coeff[0], sl.cc_coeff[1] = P(ccoef), P(cclip), P(cc), 0
    slice_idx, col_bd, row_bd = np.zeros(1, np.int16), np.array([0, 1], np.int16), np.array([0, 1], np.int16)
    for on in (0, 1):
        tab = abi.AlfCtb()
        tab.ctb_flag[0] = tab.ctb_flag[1] = tab.ctb_flag[2] = on
        tab.filt_set_idx_y, tab.alt_idx[0], tab.alt_idx[1] = 17, 3, 5
        tab.cc_idc[0], tab.cc_idc[1] = 2 * on, 1 * on           # Cr has no CC APS: stays off
        got = [np.full_like(p, 7) for p in src]
        f = abi.AlfFrame()
        for c in range(3):
            f.dst[c], f.src[c], f.dst_stride[c], f.src_stride[c] = P(got[c]), P(src[c]), dims[c][0] * isz, dims[c][0] * isz
        f.alf, f.slices, f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = ctypes.addressof(tab), ctypes.addressof(sl), P(slice_idx), P(col_bd), P(row_bd)
        f.width, f.height, f.ctb_width, f.ctb_height, f.ctb_log2, f.hs, f.vs, f.n_comp = w, h, 1, 1, 6, 1, 1, 3
        f.lfase = f.lfate = 1
        orc.orc_alf_frame_pass(bd, ctypes.byref(f))
        if not on:
            assert all(np.array_equal(got[c], src[c]) for c in range(3))
            continue
        pad = [np.pad(p, 8, mode="edge") for p in src]
        pw = [p.shape[1] for p in pad]
        want = [np.zeros_like(p) for p in src]
        nblk = (w // 4) * (h // 4)
        cls, tr, grad = np.zeros(nblk, np.int32), np.zeros(nblk, np.int32), np.zeros((h + 8) * (w + 8), np.int32)
        cf, cl = np.zeros((nblk, 12), np.int16), np.zeros((nblk, 12), np.int16)
        c2f = np.ctypeslib.as_array((ctypes.c_uint8 * 25).in_dll(orc, "orc_tab_alf_aps_class_to_filt_map"))
        orc.orc_alf_classify(bd, P(cls), P(tr), P(pad[0], 8 * pw[0] + 8), pw[0] * isz, w, h, 60, P(grad))
        orc.orc_alf_recon_coeff_and_clip(bd, P(cf), P(cl), P(cls), P(tr), nblk, P(coeff), P(clipi), P(c2f))
        orc.orc_alf_filter_luma(bd, P(want[0]), w * isz, P(pad[0], 8 * pw[0] + 8), pw[0] * isz, w, h, P(cf), P(cl), 60)
        clipv = np.array([1 << bd, 1 << (bd - 3), 1 << (bd - 5), 1 << (bd - 7)], np.int16)
        for c in (1, 2):
            alt = tab.alt_idx[c - 1]
            cv = clipv[cclip[alt]].copy()
            orc.orc_alf_filter_chroma(bd, P(want[c]), dims[c][0] * isz, P(pad[c], 8 * pw[c] + 8), pw[c] * isz, dims[c][0], dims[c][1],
                                      P(ccoef, alt * 6), P(cv), 30)
        orc.orc_alf_filter_cc(bd, P(want[1]), dims[1][0] * isz, P(pad[0], 8 * pw[0] + 8), pw[0] * isz, dims[1][0], dims[1][1], 1, 1,
                              P(cc, 7), 60)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), f"component {c}"


def test_deblock_bs_oracle_rules(orc):
    """orc_deblock_bs_pass (vvc_deblock_bs restated, vvc_filter.c:308-783) on synthetic side tables: entries appear only on
    transform-unit or sub-block edges; intra on either side gives 2; an all-intra picture has no strength-1 chroma entry without
    coded flags; slice edges that must not be filtered stay 0."""
    import bs_cases
    rng = np.random.default_rng(0xB5)
    t = bs_cases.BsTables(rng, 264, 136, 6, n_slices=3, tiles=False, lfase=0, lfate=1)
    out = bs_cases.run_oracle(orc, t)
    ys, xs = np.mgrid[0:t.th, 0:t.tw]
    # vertical edges: a non-zero luma entry sits on a transform-unit origin column or inside a sub-block coding block
    on_tu = t.tbx0 == xs * 4
    cbo = (t.tby0 // 4, t.tbx0 // 4)
    sb = (t.msf[cbo] | t.iaf[cbo]).astype(bool)
    assert not np.any((out["bs10"] > 0) & ~on_tu & ~sb)
    assert not np.any((out["p1"] > 0) & ~on_tu & ~sb)
    # intra on either side of a transform-unit edge: 2, unless both sides are pcm
    left_pf = np.roll(t.mvf["pred_flag"], 1, axis=1)
    edge = on_tu & (xs > 0)
    ctb_cols = (xs * 4) % 64 == 0
    slice_of = t.slice_idx.reshape(t.ch, t.cw)[ys * 4 // 64, xs * 4 // 64]
    slice_left = np.roll(slice_of, 1, axis=1)
    off = ctb_cols & (slice_of != slice_left)
    both_pcm = (t.pcm0 & np.roll(t.pcm0, 1, axis=1)).astype(bool)
    sel = edge & ~off & ~both_pcm & ((t.mvf["pred_flag"] == 0) | (left_pf == 0))
    assert np.all(out["bs10"][sel] == 2) and sel.sum() > 50
    assert np.all(out["bs10"][edge & off] == 0) and (edge & off).sum() > 0
    assert np.all(out["bs10"][:, 0] == 0) and np.all(out["bs00"][0, :] == 0)

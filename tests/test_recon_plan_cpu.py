"""CPU: vvc355_recon_plan_host — the plan the RECON walk's window load makes of a command (ffvvc_amd/csrc/recon_plan.hpp), the same
text the device runs one command per lane.  Its fields against the oracle's own derivations (orc_intra_wide_angle, orc_intra_pred_angle,
orc_intra_inv_angle, orc_intra_nscale, orc_intra_need_pdpc, orc_intra_ref_filter_flag) and, for the lengths of the reference arrays,
against the formulas of prepare_intra_edge_params (vvc_intra_template.c:467-592) written out below.  A wrong plan can send the walk's
wave into a longer loop than its edge arrays hold, so this runs before any GPU run of the pass."""
import ctypes
import itertools

import numpy as np
import pytest

from ffvvc_amd import abi
from recon_cases import CMD

PDPC, SMOOTH, FILTER, UP_LEFT, STRIP, MIP, MIP_T, QUADS, DIRECTIONAL, TWIN = (1 << i for i in range(10))
PITCH = (136, 68)          # the walk's tile pitches (luma, chroma)
SIZES = (4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(abi.LIB_PATH)
    lib.vvc355_recon_plan_host.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_void_p]
    lib.vvc355_recon_plan_host.restype = None
    return lib


def plans_of(lib, cmds, hs, vs, ctb_log2=7, tile=1, ctx=(1, 1, 1, 0, 0)):
    cmds = np.ascontiguousarray(cmds)
    assert cmds.dtype.itemsize == 40
    out = np.zeros((len(cmds), 10), np.uint32)
    cx = np.array(ctx, np.int32)
    lib.vvc355_recon_plan_host(cmds.ctypes.data, len(cmds), hs, vs, ctb_log2, PITCH[0], PITCH[1], tile, cx.ctypes.data, out.ctypes.data)
    return out


def fields(p):
    """A PRED plan's fields (recon_plan.hpp)."""
    s16 = lambda v: v.astype(np.uint16).view(np.int16).astype(np.int64)
    s8 = lambda v: v.astype(np.uint8).view(np.int8).astype(np.int64)
    p = p.astype(np.int64)
    return dict(src_off=p[:, 0].astype(np.uint32).view(np.int32).astype(np.int64), x=s16(p[:, 1] & 0xffff), w=(p[:, 1] >> 16) & 0xff, h=p[:, 1] >> 24,
                angle=s16(p[:, 2] & 0xffff), inv=s16(p[:, 2] >> 16), uleft=p[:, 3] & 0xffff, utop=p[:, 3] >> 16, la=p[:, 4] & 0xffff, ta=p[:, 4] >> 16,
                refw=p[:, 5] & 0xffff, refh=p[:, 5] >> 16, mode=s8(p[:, 6] & 0xff), kind=(p[:, 6] >> 8) & 0xff, c_idx=(p[:, 6] >> 16) & 0xff,
                ref_idx=p[:, 6] >> 24, left_size=p[:, 7] & 0xffff, top_size=p[:, 7] >> 16, nscale=s8(p[:, 8] & 0xff), mip_mode=(p[:, 8] >> 8) & 0xff,
                flags=(p[:, 8] >> 16) & 0x3ff, variant=(p[:, 8] >> 26) & 7, ref_line=s8(p[:, 9] & 0xff))


def coding_blocks(c_idx, isp, w, h, hs, vs):
    """The coding-block sizes (luma samples) a w x h prediction unit (component samples) can belong to."""
    if c_idx or not isp:
        return [(w << (hs if c_idx else 0), h << (vs if c_idx else 0))]
    if isp == 1:        # horizontal split: two or four sub-partitions on top of each other
        return [(w, k * h) for k in (2, 4) if k * h <= 64]
    out = [(k * w, h) for k in (2, 4) if k * w <= 64]
    if w == 4:          # the 4-wide prediction units of 1- and 2-sample-wide sub-partitions (get_luma_predict_unit, vvc_intra.c:216-226)
        out = [(4, h), (8, h)] + out
    return out


# ref_idx (every value the walk's ref_line accepts), bdpcm_flag, is_mip
TOOLS = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 1))
X0, Y0 = 64, 32            # luma position inside the CTU, off its edges


def pred_cases(hs, vs, c_list):
    rows = []
    for c_idx, w, h, isp in itertools.product(c_list, SIZES, SIZES, (0, 1, 2)):
        for cbw, cbh in coding_blocks(c_idx, isp, w, h, hs, vs):
            for mode, (ref_idx, bdpcm, mip) in itertools.product(range(67), TOOLS):
                if mip and mode:            # a MIP block is parsed with mode 0 (recon_cases._intra_cu)
                    continue
                if c_idx and ref_idx:       # the walk takes ref_idx 0 for chroma whatever the command says: covered by test_chroma_ref_idx
                    continue
                rows.append((c_idx, w, h, isp, cbw, cbh, mode, ref_idx, bdpcm, mip))
    return np.array(rows, np.int64)


def check_pred(lib, orc, hs, vs, c_list):
    r = pred_cases(hs, vs, c_list)
    c_idx, w, h, isp, cbw, cbh, mode, ref_idx, bdpcm, mip = r.T
    n = len(r)
    shx, shy = np.where(c_idx > 0, hs, 0), np.where(c_idx > 0, vs, 0)
    # availability answers 0 / partial / full, each side on its own cycle
    k = np.arange(n)
    left_avail = np.choose(k % 3, [0, np.maximum(1, h // 2), 600])
    top_avail = np.choose((k // 3) % 3, [600, 0, np.maximum(1, w // 2)])
    cmds = np.zeros(n, CMD)
    cmds["x0"], cmds["y0"], cmds["w"], cmds["h"] = X0, Y0, w << shx, h << shy
    cmds["cu_x0"], cmds["cu_y0"], cmds["cb_width"], cmds["cb_height"] = X0, Y0, cbw, cbh
    cmds["mode"], cmds["kind"], cmds["c_idx"], cmds["ref_idx"] = mode, abi.RECON_PRED, c_idx, ref_idx
    cmds["is_mip"], cmds["mip_mode"], cmds["mip_transposed"], cmds["isp_split"], cmds["bdpcm_flag"] = mip, 5 * mip, mip * (k & 1), isp, bdpcm
    raw = cmds.view(np.uint32).reshape(n, 10)
    raw[:, 9] = left_avail.astype(np.uint32) | (top_avail.astype(np.uint32) << 16)
    # one command per call slot: never a twin here (no two consecutive rows differ in c_idx only: the mode or the tools change)
    f = fields(plans_of(lib, cmds, hs, vs))
    assert not (f["flags"] & TWIN).any()

    # the oracle's derivations, memoised over their small domains
    memo = {}

    def table(fn, *cols):
        out = np.zeros(n, np.int64)
        for i, key in enumerate(zip(*(c.tolist() for c in cols))):
            v = memo.get((fn, key))
            if v is None:
                v = memo[(fn, key)] = getattr(orc, fn)(*key)
            out[i] = v
        return out
    for fn in ("orc_intra_wide_angle", "orc_intra_pred_angle", "orc_intra_inv_angle", "orc_intra_nscale", "orc_intra_need_pdpc", "orc_intra_ref_filter_flag"):
        getattr(orc, fn).restype = ctypes.c_int
    m2 = table("orc_intra_wide_angle", isp, c_idx, w, h, cbw, cbh, mode)
    directional = (mip == 0) & ~np.isin(m2, (0, 1, 18, 50))
    angle = np.where(directional, table("orc_intra_pred_angle", m2), 0)
    inv = np.where(directional, table("orc_intra_inv_angle", np.where(directional, angle, 1)), 0)
    need_pdpc = table("orc_intra_need_pdpc", w, h, bdpcm, m2, ref_idx)
    nscale = table("orc_intra_nscale", w, h, np.where(directional & ((m2 < 18) | (m2 > 50)), m2, 0))
    rff = np.where(mip == 1, 0, table("orc_intra_ref_filter_flag", m2))
    # prepare_intra_edge_params (vvc_intra_template.c:467-592)
    smooth = (ref_idx == 0) & (w * h > 32) & (c_idx == 0) & (isp == 0) & (rff != 0)                       # :479
    planar = (mip == 1) | (m2 == 0)
    split_ref = (isp != 0) & (c_idx == 0)
    refw = np.where(split_ref, cbw + w, 2 * w)                                                             # :510-516
    refh = np.where(split_ref, cbh + h, 2 * h)
    left_size = np.select([planar, m2 == 1, m2 == 50, m2 == 18], [h + 1, h, np.where(need_pdpc != 0, h, 1), h], refh)      # :493-521
    top_size = np.select([planar, m2 == 1, m2 == 50, m2 == 18], [w + 1, w, w, np.where(need_pdpc != 0, w, 1)], refw)
    uleft, utop = left_size + (planar & smooth), top_size + (planar & smooth)
    log2 = lambda v: np.log2(v).astype(np.int64)
    thres = np.array([24, 14, 2, 0, 0])[((log2(w) + log2(h)) >> 1) - 2]                                    # :558-561
    filter_flag = directional & ~((rff != 0) | (ref_idx != 0) | (isp != 0)) & (np.minimum(abs(m2 - 50), abs(m2 - 18)) > thres)

    def same(name, want, where=None):
        got = f[name]
        bad = (got != want) if where is None else ((got != want) & where)
        assert not bad.any(), (name, r[np.argmax(bad)].tolist(), int(got[np.argmax(bad)]), int(np.broadcast_to(want, got.shape)[np.argmax(bad)]))
    same("kind", abi.RECON_PRED); same("c_idx", c_idx); same("ref_idx", ref_idx)
    same("x", X0 >> shx); same("w", w); same("h", h)
    same("src_off", (Y0 >> shy) * np.where(c_idx > 0, PITCH[1], PITCH[0]) + (X0 >> shx))
    same("mode", m2)
    same("angle", angle); same("inv", inv)
    fl = f["flags"]
    for bit, want, name in ((PDPC, need_pdpc != 0, "need_pdpc"), (SMOOTH, smooth, "rff && smooth"), (FILTER, filter_flag, "filter_flag"), (MIP, mip == 1, "is_mip"),
                            (DIRECTIONAL, directional, "directional"), (MIP_T, (mip == 1) & ((k & 1) == 1), "mip_transposed"),
                            (UP_LEFT, np.ones(n, bool), "cand_up_left"), (STRIP, np.zeros(n, bool), "strip")):
        bad = ((fl & bit) != 0) != want
        assert not bad.any(), (name, r[np.argmax(bad)].tolist())
    same("nscale", nscale, directional & (need_pdpc != 0))
    same("mip_mode", 5 * mip)
    same("ref_line", np.where(ref_idx == 3, -4, -1 - ref_idx))                                             # :486
    same("left_size", left_size); same("top_size", top_size); same("uleft", uleft); same("utop", utop)
    same("refw", refw, directional); same("refh", refh, directional)
    same("la", np.minimum(uleft, left_avail)); same("ta", np.minimum(utop, top_avail))                    # :523, :527: a request of the unfiltered size
    # what the walk's lanes may touch: the edge arrays hold 6 * 64 + 5 entries around origin 64 + 3
    assert (uleft + 4 <= 6 * 64 + 5 - 67).all() and (utop + 4 <= 6 * 64 + 5 - 67).all()
    # the predictor's choice (intra.hip, intra_pred_run): four samples per lane for blocks of more than two steps of the wave
    quads = (w * h > 128) & (w >= 4) & (~directional | (m2 >= 34) | (h >= 4))
    assert (((fl & QUADS) != 0) == quads).all()
    variant = np.where(directional, (m2 >= 34) * 4 + (c_idx == 0) * 2 + (need_pdpc != 0),
                       np.select([m2 == 0, m2 == 1, m2 == 50], [0, 1, 2], 3) * 2 + (need_pdpc != 0))
    same("variant", variant, mip == 0)
    return n


def test_luma_plans(lib, orc):
    assert check_pred(lib, orc, 1, 1, (0,)) > 30000


@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (0, 0)])
def test_chroma_plans(lib, orc, hs, vs):
    assert check_pred(lib, orc, hs, vs, (1, 2)) > 20000


def _cmd(**kw):
    c = np.zeros(1, CMD)
    for k, v in kw.items():
        c[k] = v
    return c


def test_chroma_ref_idx_is_zero(lib):
    """intra_pred takes the reference line of luma blocks only (vvc_intra_template.c:610): a chroma command's ref_idx does not count."""
    c = _cmd(kind=abi.RECON_PRED, c_idx=1, x0=64, y0=32, w=16, h=16, cb_width=16, cb_height=16, mode=30, ref_idx=2)
    f = fields(plans_of(lib, c, 1, 1))
    assert f["ref_idx"][0] == 0 and f["ref_line"][0] == -1


def test_strip_and_up_left(lib):
    """The strip flag (the block sits on the CTU's top edge, tile walks only) and ff_vvc_set_neighbour_available's cand_up_left
    (vvc_ctu.c:2497-2510), for the CTU's corner, its edges and its inside, with and without neighbour CTUs."""
    for ctb_log2, hs, vs in ((7, 1, 1), (6, 1, 1), (5, 1, 1), (7, 0, 0)):
        ctb = 1 << ctb_log2
        for up, left, tile, c_idx in itertools.product((0, 1), (0, 1), (0, 1), (0, 1)):
            ox, oy = 2 * ctb, ctb
            pos = [(ox, oy), (ox + 8, oy), (ox, oy + 8), (ox + 8, oy + 16)]
            cmds = np.concatenate([_cmd(kind=abi.RECON_PRED, c_idx=c_idx, x0=x, y0=y, w=8, h=8, cb_width=8, cb_height=8, mode=1) for x, y in pos])
            f = fields(plans_of(lib, cmds, hs, vs, ctb_log2, tile, (up, left, up & left, ox, oy)))
            want_ul = [up & left, up, left, 1]
            want_strip = [tile, tile, 0, 0]
            assert [int(v != 0) for v in f["flags"] & UP_LEFT] == want_ul
            assert [int(v != 0) for v in f["flags"] & STRIP] == want_strip


def test_twin(lib):
    """Cb and Cr of a coding unit — consecutive PREDs that differ in c_idx only — carry the twin bit on Cb (tile walks only), and the
    pair's predictor choice is the half wave's (w * h > 64)."""
    def pair(**kw):
        a = dict(kind=abi.RECON_PRED, x0=64, y0=32, w=32, h=16, cu_x0=64, cu_y0=32, cb_width=32, cb_height=16, mode=50)
        b = dict(a)
        b.update(kw)
        return np.concatenate([_cmd(c_idx=1, **a), _cmd(c_idx=2, **b)])
    f = fields(plans_of(lib, pair(), 1, 1))           # chroma 16 x 8 = 128 samples: quads for the half wave, not for the whole
    assert [int(v != 0) for v in f["flags"] & TWIN] == [1, 0]
    assert [int(v != 0) for v in f["flags"] & QUADS] == [1, 0]
    assert not (fields(plans_of(lib, pair(), 1, 1, tile=0))["flags"] & TWIN).any()
    for other in (dict(mode=18), dict(w=16), dict(cu_x0=32), dict(cb_height=32), dict(is_mip=1), dict(bdpcm_flag=1)):
        assert not (fields(plans_of(lib, pair(**other), 1, 1))["flags"] & TWIN).any(), other
    luma_pair = np.concatenate([_cmd(kind=abi.RECON_PRED, c_idx=0, x0=64, y0=32, w=8, h=8), _cmd(kind=abi.RECON_PRED, c_idx=2, x0=64, y0=32, w=8, h=8)])
    assert not (fields(plans_of(lib, luma_pair, 1, 1))["flags"] & TWIN).any()


def test_resid_ciip_cclm_plans(lib):
    hs = vs = 1
    for ctb_log2 in (5, 7):
        size_y = min(1 << ctb_log2, 64)
        for c_idx, (w, h), joint in itertools.product((0, 1, 2), ((1, 16), (2, 8), (4, 4), (8, 32), (64, 64)), (0, 8, 1 | 2 | 4 | 8)):
            # RESID: w, h in component samples, position in luma samples
            c = _cmd(kind=abi.RECON_RESID, c_idx=c_idx, x0=200, y0=72, w=w, h=h, cu_x0=196, cu_y0=72, joint=joint, resid=0x123456789ab0)
            raw = c.view(np.uint32).reshape(1, 10).copy()
            raw[0, 8] |= 3 << 16                     # the pre-pass's answers
            p = plans_of(lib, raw.view(CMD).reshape(1), hs, vs, ctb_log2)[0].astype(np.int64)
            sh = 1 if c_idx else 0
            assert (p[[0, 1, 3, 6, 8, 9]] == raw[0, [0, 1, 3, 6, 8, 9]]).all()
            assert p[2] == (72 >> sh) * PITCH[1 if c_idx else 0] + (200 >> sh)
            assert p[4] == (int(np.log2(w)) | c_idx << 8 | joint << 16 | (1 << 24 if joint & 8 else 0)) and p[5] == w * h
            assert p[7] == ((196 & ~(size_y - 1)) | (72 & ~(size_y - 1)) << 16)
        for c_idx, (w, h) in itertools.product((0, 1, 2), ((8, 8), (32, 16), (64, 64))):
            # CIIP: w, h of the coding unit in luma samples
            c = _cmd(kind=abi.RECON_CIIP, c_idx=c_idx, x0=192, y0=64, w=w, h=h, cu_x0=192, cu_y0=64, joint=3, resid=0x1000)
            raw = c.view(np.uint32).reshape(1, 10)
            p = plans_of(lib, c, hs, vs, ctb_log2)[0].astype(np.int64)
            sh = 1 if c_idx else 0
            assert (p[[0, 1, 3, 6]] == raw[0, [0, 1, 3, 6]]).all()
            assert p[2] == (64 >> sh) * PITCH[1 if c_idx else 0] + (192 >> sh)
            assert p[4] == (int(np.log2(w >> sh)) | c_idx << 8 | 3 << 16) and p[5] == (w >> sh) * (h >> sh)
        for y0, bits in itertools.product((128, 136), (0, 1, 2, 3)):
            c = _cmd(kind=abi.RECON_CCLM, c_idx=1, x0=64, y0=y0, w=16, h=16, cu_x0=64, cu_y0=y0, mode=82)
            raw = c.view(np.uint32).reshape(1, 10).copy()
            raw[0, 8] |= bits << 16
            raw[0, 9] = 24 | 40 << 16
            p = plans_of(lib, raw.view(CMD).reshape(1), hs, vs, ctb_log2)[0].astype(np.int64)
            assert (p[[2, 3, 6, 9]] == raw[0, [2, 3, 6, 9]]).all()
            boundary = int(y0 % (1 << ctb_log2) == 0)
            assert p[7] == ((bits & 1) | (bits >> 1) << 8 | boundary << 16)

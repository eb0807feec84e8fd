"""Pictures, frames, host runs and digests for the in-loop filter passes pinned against the reference's own callers (oracle/ref_shim_filter.c:
ff_vvc_deblock_vertical / _horizontal, ff_vvc_sao_filter, ff_vvc_alf_filter on real contexts): deblocking pictures D0-D14, SAO / ALF pictures
F0-F4, the chained picture C0 and the freshly drawn pictures of the sweep.  Every picture is deterministic: a smooth picture plus per-4x4 steps
(noise planes switch nearly every luma decision off; D14 alone has one step per coding block, for the long luma filters), side tables from bs_cases.BsTables, QP tables constant per unit, painted from sidecars
(qp_rec_cases.expected) so that the record passes can reproduce them.  Used by tests/test_ref_passes_cpu.py, tests/test_ref_passes_gpu.py and
tools/gen_golden.py; tests/golden/ref_passes.json holds the reference's digests."""
import ctypes
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np

import bipred_cases as bc
import bs_cases
import bs_rec_cases as rc
import qp_rec_cases as qc
from ffvvc_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_passes.json")
SEED = 0x5EED0F00
ALF_LUMA_SETS = 7                              # luma sets per slice that ref_alf_picture's APS mapping carries (ref_alf_luma_sets())
QP_TABLES = qc.TABLES                          # qp_y, qp_c0, qp_c1

DEBLOCK = [f"D{i}" for i in range(15)]
FILTER = [f"F{i}" for i in range(5)]
CHAIN = "C0"
REC_PATH = [n for n in DEBLOCK if n != "D13"]  # D13 (minimum coding block 8) has no record path: the record passes require 4

# D8-D12: bit depth, (hs, vs), n_comp, CTU log2, size, (lfase, lfate), LADF
_WIDE = [
    dict(bd=8, fmt=(1, 1), n_comp=3, ctb_log2=5, size=(200, 328), lf=(0, 0), ladf=True),
    dict(bd=12, fmt=(1, 1), n_comp=3, ctb_log2=7, size=(264, 136), lf=(1, 0), ladf=True),
    dict(bd=12, fmt=(1, 0), n_comp=3, ctb_log2=5, size=(264, 136), lf=(0, 1), ladf=True),
    dict(bd=8, fmt=(0, 0), n_comp=3, ctb_log2=6, size=(200, 328), lf=(1, 1), ladf=False),
    dict(bd=10, fmt=(1, 1), n_comp=1, ctb_log2=6, size=(264, 136), lf=(0, 0), ladf=True),
]
# F0-F4 at 328x200: bit depth, (hs, vs), n_comp, CTU log2, (lfase, lfate)
_FILTER = [
    dict(bd=10, fmt=(1, 1), n_comp=3, ctb_log2=6, lf=(0, 0)),
    dict(bd=8, fmt=(1, 1), n_comp=3, ctb_log2=7, lf=(1, 0)),
    dict(bd=10, fmt=(0, 0), n_comp=3, ctb_log2=5, lf=(0, 1)),
    dict(bd=12, fmt=(1, 0), n_comp=3, ctb_log2=6, lf=(1, 1)),
    dict(bd=10, fmt=(1, 1), n_comp=1, ctb_log2=6, lf=(0, 0)),
]


def px(bd):
    return np.uint8 if bd == 8 else np.uint16


def stepped_planes(rng, dims, bd):
    """The plane recipe of qp_rec_cases.e2e_inputs at any depth: band-limited content plus one step per 4x4 unit."""
    planes = []
    for (pw, ph) in dims:
        base = bc.smooth_picture(rng, ph, pw, bd, scale=32).astype(np.int64)
        offs = rng.integers(-(1 << (bd - 6)), (1 << (bd - 6)) + 1, size=(ph // 4, pw // 4))
        planes.append(np.clip(base + np.kron(offs, np.ones((4, 4), np.int64)), 0, (1 << bd) - 1).astype(px(bd)))
    return planes


def block_planes(rng, t, dims, bd):
    """Hand-placed content for the long luma filters, which per-4x4 steps switch off (their decision wants both sides of the edge smooth over
    seven samples): a gentle ramp plus one step per CODING BLOCK, no noise.  Inside a block the second differences vanish."""
    off_u = rng.integers(-(1 << (bd - 7)), (1 << (bd - 7)) + 1, size=(t.th, t.tw))[t.cby // 4, t.cbx // 4]
    ys, xs = np.arange(t.height)[:, None], np.arange(t.width)[None, :]
    luma = (1 << (bd - 1)) + ((xs + ys) >> 2) - ((t.width + t.height) >> 3) + np.kron(off_u, np.ones((4, 4), np.int64))
    planes = [luma] + [luma[::1 << t.vs, ::1 << t.hs] + k for k in (3, -5)][:len(dims) - 1]
    return [np.ascontiguousarray(np.clip(p, 0, (1 << bd) - 1).astype(px(bd))) for p in planes]


def plane_dims(t, n_comp):
    return [(t.width, t.height)] + [(t.width >> t.hs, t.height >> t.vs)] * (n_comp - 1)


# ---------------------------------------------------------------------------------------------------------------- deblocking pictures

def _finish_deblock(name, bd, n_comp, t, planes, qp, dbp, ladf, rec, min_cb_log2=2):
    arrays = {n: getattr(t, n) for n in t.IN}
    arrays.update({n: np.ascontiguousarray(qp[n]) for n in QP_TABLES})
    arrays["dbp"] = dbp
    min_cb_width = t.tw
    if min_cb_log2 == 3:
        # every leaf of the generator is at least 8 wide and 8-aligned: the 8x8 grid holds the same information
        for n in ("cbx", "cby", "cbw", "cbh", "msf", "iaf", "qp_y"):
            full = arrays[n]
            assert np.array_equal(np.repeat(np.repeat(full[::2, ::2], 2, 0), 2, 1)[:full.shape[0], :full.shape[1]], full), n
            arrays[n] = np.ascontiguousarray(full[::2, ::2])
        min_cb_width = (t.width + 7) // 8
        assert arrays["cbx"].shape[1] == min_cb_width
    return SimpleNamespace(name=name, bd=bd, n_comp=n_comp, t=t, planes=planes, dims=plane_dims(t, n_comp), arrays=arrays, ladf=ladf, rec=rec,
                           min_cb_log2=min_cb_log2, min_cb_width=min_cb_width, n_slices=len(t.ref_poc))


def draw_deblock(name, rng, bd, fmt, n_comp, ctb_log2, size, n_slices, tiles, lf, ladf, min_cb_log2=2, split=(0.75, 0.35), blocks=False):
    """A picture over the whole domain the table setters can write (vvc_ctu.c:173-209): QpY in -QpBdOffset..63, chroma QP in 0..63 + QpBdOffset,
    even per-CTU beta / tc offsets in -24..24, and (ladf) five LADF intervals whose bounds are quantiles of the luma plane."""
    qp_bd = 6 * (bd - 8)
    t = bs_cases.BsTables(rng, size[0], size[1], ctb_log2, n_slices=n_slices, tiles=tiles, lfase=lf[0], lfate=lf[1], hs=fmt[0], vs=fmt[1], split=split)
    (cu, cu_first), (tu, tu_first), _ = rc.grouped(t)
    rec = qc.Pic(g=t, cu=cu, tu=tu, cu_first=cu_first, tu_first=tu_first, cu_qp=rng.integers(-qp_bd, 64, size=len(cu)).astype(np.int8),
                 tu_qp_c=rng.integers(0, 64 + qp_bd, size=(len(tu), 2)).astype(np.int8))
    planes = block_planes(rng, t, plane_dims(t, n_comp), bd) if blocks else stepped_planes(rng, plane_dims(t, n_comp), bd)
    dbp = (2 * rng.integers(-12, 13, size=(t.cw * t.ch, 6))).astype(np.int8)
    conf = None
    if ladf:
        bounds = [0] + [int(v) for v in np.quantile(planes[0], [0.2, 0.4, 0.6, 0.8])]
        assert all(a < b for a, b in zip(bounds, bounds[1:])), bounds
        conf = dict(bounds=bounds, lowest=int(rng.integers(-12, 13)), offsets=[int(v) for v in rng.integers(-12, 13, size=4)])
    return _finish_deblock(name, bd, n_comp, t, planes, qc.expected(rec), dbp, conf, rec if min_cb_log2 == 2 else None, min_cb_log2)


_deblock = {}


def deblock_picture(orc, name):
    """D0-D7: bs_rec_cases.CASES with exactly the inputs of test_deblock_qp_rec_* (10 bit, LADF off); D8-D12: the wider domain; D13:
    minimum coding block 8; D14: block-wise smooth content (the per-4x4 steps of the others never let a long luma filter run).  Made once per
    process; nobody writes to a picture."""
    if name not in _deblock:
        i = int(name[1:])
        if i < 8:
            t, _ = rc.case(orc, i)
            planes, _dims, dbp = qc.e2e_inputs(orc, i)
            rec = qc.picture(orc, i)
            _deblock[name] = _finish_deblock(name, qc.BD, 3, t, planes, qc.expected(rec), dbp, None, rec)
        elif i < 13:
            c = _WIDE[i - 8]
            _deblock[name] = draw_deblock(name, np.random.default_rng(SEED + i), c["bd"], c["fmt"], c["n_comp"], c["ctb_log2"], c["size"], 4, True,
                                          c["lf"], c["ladf"])
        elif i == 13:
            _deblock[name] = draw_deblock(name, np.random.default_rng(SEED + i), 10, (1, 1), 3, 6, (264, 136), 3, True, (1, 1), True, min_cb_log2=3)
        else:                                  # D14, hand-placed: large blocks with smooth insides, for the long luma filters
            _deblock[name] = draw_deblock(name, np.random.default_rng(SEED + i), 10, (1, 1), 3, 7, (264, 136), 2, False, (1, 1), False,
                                          split=(0.35, 0.1), blocks=True)
    return _deblock[name]


def sweep_deblock(k):
    """Picture k of the sweep: geometry, format, depth, flags and seed drawn from k."""
    rng = np.random.default_rng(SEED + 1000 + k)
    fmt, n_comp = [((1, 1), 3), ((1, 0), 3), ((0, 0), 3), ((1, 1), 1)][int(rng.integers(0, 4))]
    size = (8 * int(rng.integers(5, 34)), 8 * int(rng.integers(5, 18)))
    return draw_deblock(f"sweep-deblock-{k}", rng, int(rng.choice([8, 10, 12])), fmt, n_comp, int(rng.integers(5, 8)), size, int(rng.integers(1, 6)),
                        bool(rng.integers(0, 2)), (int(rng.integers(0, 2)), int(rng.integers(0, 2))), bool(rng.integers(0, 4)),
                        min_cb_log2=3 if rng.integers(0, 4) == 0 else 2, split=(float(rng.choice([0.6, 0.75, 0.9])), float(rng.choice([0.2, 0.35, 0.5]))))


def bs_frame(pic, addr):
    f = pic.t.frame(addr)
    f.n_comp, f.min_cb_log2, f.min_cb_width = pic.n_comp, pic.min_cb_log2, pic.min_cb_width
    return f


def deblock_frame(pic, vertical, planes, strides, addr):
    """abi.DeblockFrame of one pass: addr(name) = address of a table of pic.arrays or of an output table (BsTables names)."""
    t, f = pic.t, abi.DeblockFrame()
    for c in range(pic.n_comp):
        f.plane[c], f.stride[c], f.bs[c] = planes[c], strides[c], addr(f"bs{vertical}{c}")
    f.max_len_p, f.max_len_q, f.qp_y, f.db_params = addr(f"p{vertical}"), addr(f"q{vertical}"), addr("qp_y"), addr("dbp")
    if pic.n_comp == 3:
        f.tb_size_c, f.qp_c[0], f.qp_c[1] = addr("tbw1" if vertical else "tbh1"), addr("qp_c0"), addr("qp_c1")
    f.width, f.height, f.min_tu_width, f.min_cb_width, f.ctb_width = t.width, t.height, t.tw, pic.min_cb_width, t.cw
    f.min_cb_log2, f.ctb_log2, f.hs, f.vs, f.n_comp, f.vertical = pic.min_cb_log2, t.ctb_log2, t.hs, t.vs, pic.n_comp, vertical
    f.qp_bd_offset = 6 * (pic.bd - 8)
    if pic.ladf:
        f.ladf_enabled, f.num_ladf_intervals, f.ladf_lowest_qp_offset = 1, 5, pic.ladf["lowest"]
        for k in range(5):
            f.ladf_lower_bound[k] = pic.ladf["bounds"][k]
        for k in range(4):
            f.ladf_qp_offset[k] = pic.ladf["offsets"][k]
    return f


def _proto(lib, name, *args):
    fn = getattr(lib, name)
    fn.argtypes, fn.restype = list(args), (ctypes.c_int if name.startswith("ref_") else None)
    return fn


def run_deblock(lib, side, pic, planes=None):
    """Boundary strengths, then vertical and horizontal edges, on the host by the reference ("ref": ref_deblock_picture) or the oracle ("orc":
    orc_deblock_bs_pass + orc_deblock_frame_pass x 2).  Returns {table name: uint8 (th, tw)} for BsTables.OUT — both sides start from zero
    tables — plus "v" and "h": the planes after either pass."""
    t = pic.t
    a = {n: v.copy() for n, v in pic.arrays.items()}
    for n in t.OUT:
        a[n] = np.zeros((t.th, t.tw), np.uint8)
    addr = lambda n: a[n].ctypes.data          # noqa: E731
    src = planes if planes is not None else pic.planes
    out = {}
    if side == "orc":
        work = [p.copy() for p in src]
        _proto(lib, "orc_deblock_bs_pass", ctypes.POINTER(abi.BsFrame))(ctypes.byref(bs_frame(pic, addr)))
        fn = _proto(lib, "orc_deblock_frame_pass", ctypes.c_int, ctypes.POINTER(abi.DeblockFrame))
        for vertical in (1, 0):
            fn(pic.bd, ctypes.byref(deblock_frame(pic, vertical, [p.ctypes.data for p in work], [p.strides[0] for p in work], addr)))
            out["v" if vertical else "h"] = [p.copy() for p in work]
    else:
        fn = _proto(lib, "ref_deblock_picture", ctypes.c_int, ctypes.POINTER(abi.BsFrame), ctypes.POINTER(abi.DeblockFrame), ctypes.c_int, ctypes.c_int)
        for only_v in (1, 0):
            work = [p.copy() for p in src]
            f = deblock_frame(pic, 1, [p.ctypes.data for p in work], [p.strides[0] for p in work], addr)
            err = fn(pic.bd, ctypes.byref(bs_frame(pic, addr)), ctypes.byref(f), pic.n_slices, only_v)
            assert err == 0, f"{pic.name}: ref_deblock_picture refused the picture"
            out["v" if only_v else "h"] = work
    for n, v in pic.arrays.items():
        assert np.array_equal(a[n].view(np.uint8), v.view(np.uint8)), f"{pic.name}: {side} wrote to the input table {n}"
    out.update({n: a[n] for n in t.OUT})
    return out


# ---------------------------------------------------------------------------------------------------------------- SAO / ALF pictures

def draw_filter(name, rng, bd, fmt, n_comp, ctb_log2, size, n_slices, tiles, lf, t=None, planes=True):
    """test_chain_gpu's SAO / ALF recipe: random per-CTB SAO and ALF parameters, two luma APS sets, one chroma set, cross-component sets of
    which slice 1 has none for Cr, and slice 1 listing its luma sets in the other order."""
    if t is None:
        t = bs_cases.BsTables(rng, size[0], size[1], ctb_log2, n_slices=n_slices, tiles=tiles, lfase=lf[0], lfate=lf[1], hs=fmt[0], vs=fmt[1],
                              split=(0.9, 0.5), cbf_p=0.5)
    n_ctb = t.cw * t.ch
    dims = plane_dims(t, n_comp)
    rec = stepped_planes(rng, dims, bd) if planes else None
    sao_tab, alf_tab = (abi.SaoCtb * n_ctb)(), (abi.AlfCtb * n_ctb)()
    for i in range(n_ctb):
        for c in range(3):
            sao_tab[i].type_idx[c], sao_tab[i].band_position[c], sao_tab[i].eo_class[c] = int(rng.integers(0, 3)), int(rng.integers(0, 32)), int(rng.integers(0, 4))
            for k in range(1, 5):
                sao_tab[i].offset_val[c][k] = int(rng.integers(-(1 << (bd - 5)) + 1, 1 << (bd - 5)))
            alf_tab[i].ctb_flag[c] = int(rng.integers(0, 4) > 0)
        alf_tab[i].filt_set_idx_y = int(rng.integers(0, 18))
        for c in range(2):
            alf_tab[i].alt_idx[c], alf_tab[i].cc_idc[c] = int(rng.integers(0, 8)), int(rng.integers(0, 5))
    aps = [rng.integers(-40, 40, size=(25, 12)).astype(np.int16), rng.integers(-40, 40, size=(25, 12)).astype(np.int16),
           rng.integers(0, 4, size=(25, 12)).astype(np.uint8), rng.integers(0, 4, size=(25, 12)).astype(np.uint8),
           rng.integers(-48, 48, size=(8, 6)).astype(np.int16), rng.integers(0, 4, size=(8, 6)).astype(np.uint8),
           rng.integers(-32, 32, size=(4, 7)).astype(np.int16), rng.integers(-32, 32, size=(4, 7)).astype(np.int16)]
    sao = np.frombuffer(bytes(sao_tab), np.uint8).copy()
    alf = np.frombuffer(bytes(alf_tab), np.uint8).copy()
    luma_sets = 2
    assert luma_sets <= ALF_LUMA_SETS and int(alf.reshape(n_ctb, 8)[:, 3].max()) < 16 + luma_sets
    tiled = bool(t.col_bd[:-1].any() or t.row_bd[:-1].any())
    return SimpleNamespace(name=name, bd=bd, n_comp=n_comp, t=t, planes=rec, dims=dims, sao=sao, alf=alf, aps=aps, lfase=lf[0], lfate=lf[1],
                           no_tile_filter=int(tiled and not lf[1]), n_slices=int(t.slice_idx.max()) + 1)


_filter = {}


def filter_picture(name):
    if name not in _filter:
        i = int(name[1:])
        c = _FILTER[i]
        _filter[name] = draw_filter(name, np.random.default_rng(SEED + 100 + i), c["bd"], c["fmt"], c["n_comp"], c["ctb_log2"], (328, 200), 3, True, c["lf"])
    return _filter[name]


def sweep_filter(k):
    rng = np.random.default_rng(SEED + 2000 + k)
    fmt, n_comp = [((1, 1), 3), ((1, 0), 3), ((0, 0), 3), ((1, 1), 1)][int(rng.integers(0, 4))]
    size = (8 * int(rng.integers(5, 34)), 8 * int(rng.integers(5, 18)))
    return draw_filter(f"sweep-filter-{k}", rng, int(rng.choice([8, 10, 12])), fmt, n_comp, int(rng.integers(5, 8)), size, int(rng.integers(1, 6)),
                       bool(rng.integers(0, 2)), (int(rng.integers(0, 2)), int(rng.integers(0, 2))))


_chain = []


def chain_picture():
    """C0: (deblocking picture, SAO / ALF parameters on the same slices and tiles) of one 264x136 picture at 10 bit 4:2:0."""
    if not _chain:
        rng = np.random.default_rng(SEED + 200)
        d = draw_deblock(CHAIN, rng, 10, (1, 1), 3, 6, (264, 136), 3, True, (0, 0), True, split=(0.9, 0.5))
        _chain.append((d, draw_filter(CHAIN, rng, 10, (1, 1), 3, 6, None, 3, True, (0, 0), t=d.t, planes=False)))
    return _chain[0]


def alf_slices(fp, ap):
    """(abi.AlfSlice * n) from the addresses `ap` of fp.aps on the side that runs."""
    slices = (abi.AlfSlice * fp.n_slices)()
    for i, s in enumerate(slices):
        order = [0, 1] if i != 1 else [1, 0]
        for k in range(2):
            s.luma_coeff[k], s.luma_clip_idx[k] = ap[order[k]], ap[2 + order[k]]
        s.chroma_coeff, s.chroma_clip_idx, s.cc_coeff[0], s.cc_coeff[1] = ap[4], ap[5], ap[6], (ap[7] if i != 1 else 0)
    return slices


def _geometry(f, fp):
    t = fp.t
    f.width, f.height, f.ctb_width, f.ctb_height = t.width, t.height, t.cw, t.ch
    f.ctb_log2, f.hs, f.vs, f.n_comp, f.lfase = t.ctb_log2, t.hs, t.vs, fp.n_comp, fp.lfase


def sao_frame(fp, dst, src, dst_stride, src_stride, addr):
    """addr(name): "sao", "slice_idx", "col_bd", "row_bd"."""
    f = abi.SaoFrame()
    for c in range(fp.n_comp):
        f.dst[c], f.src[c], f.dst_stride[c], f.src_stride[c] = dst[c], src[c], dst_stride[c], src_stride[c]
    f.sao, f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = addr("sao"), addr("slice_idx"), addr("col_bd"), addr("row_bd")
    _geometry(f, fp)
    f.no_tile_filter = fp.no_tile_filter
    return f


def alf_frame(fp, dst, src, dst_stride, src_stride, addr):
    """addr(name): "alf", "slices", "slice_idx", "col_bd", "row_bd"."""
    f = abi.AlfFrame()
    for c in range(fp.n_comp):
        f.dst[c], f.src[c], f.dst_stride[c], f.src_stride[c] = dst[c], src[c], dst_stride[c], src_stride[c]
    f.alf, f.slices, f.slice_idx, f.ctb_to_col_bd, f.ctb_to_row_bd = addr("alf"), addr("slices"), addr("slice_idx"), addr("col_bd"), addr("row_bd")
    _geometry(f, fp)
    f.lfate = fp.lfate
    return f


def run_filter(lib, side, fp, stage, planes=None):
    """SAO or ALF (stage "sao" / "alf") of `planes` (default fp.planes) on the host: the reference filters a copy in place, the oracle writes
    planes pre-filled with 0x21.  Returns the filtered planes."""
    t = fp.t
    src = [p.copy() for p in (planes if planes is not None else fp.planes)]
    keep = {"sao": fp.sao.copy(), "alf": fp.alf.copy(), "slice_idx": t.slice_idx.copy(), "col_bd": t.col_bd.copy(), "row_bd": t.row_bd.copy()}
    aps = [a.copy() for a in fp.aps]
    slices = alf_slices(fp, [a.ctypes.data for a in aps])
    addr = lambda n: ctypes.addressof(slices) if n == "slices" else keep[n].ctypes.data          # noqa: E731
    dst = src if side == "ref" else [np.full_like(p, 0x21) for p in src]
    make, ty = (sao_frame, abi.SaoFrame) if stage == "sao" else (alf_frame, abi.AlfFrame)
    f = make(fp, [p.ctypes.data for p in dst], [p.ctypes.data for p in src], [p.strides[0] for p in dst], [p.strides[0] for p in src], addr)
    if side == "ref":
        err = _proto(lib, f"ref_{stage}_picture", ctypes.c_int, ctypes.POINTER(ty))(fp.bd, ctypes.byref(f))
        assert err == 0, f"{fp.name}: ref_{stage}_picture refused the picture"
    else:
        _proto(lib, f"orc_{stage}_frame_pass", ctypes.c_int, ctypes.POINTER(ty))(fp.bd, ctypes.byref(f))
    return dst


def run_chain(lib, side):
    """C0 on the host: {tables, "v", "h", "sao", "alf"}, every stage on what the previous one left."""
    d, fp = chain_picture()
    out = run_deblock(lib, side, d)
    out["sao"] = run_filter(lib, side, fp, "sao", out["h"])
    out["alf"] = run_filter(lib, side, fp, "alf", out["sao"])
    return out


# ---------------------------------------------------------------------------------------------------------------- digests

def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def deblock_inputs_digest(pic):
    t = pic.t
    conf = json.dumps([pic.bd, pic.n_comp, pic.min_cb_log2, pic.min_cb_width, t.width, t.height, t.ctb_log2, t.hs, t.vs, t.lfase, t.lfate, pic.ladf], sort_keys=True)
    return sha(np.frombuffer(conf.encode(), np.uint8), *[pic.arrays[n].view(np.uint8) for n in sorted(pic.arrays)], *pic.planes)


def filter_inputs_digest(fp, planes=True):
    t = fp.t
    conf = json.dumps([fp.bd, fp.n_comp, t.width, t.height, t.ctb_log2, t.hs, t.vs, fp.lfase, fp.lfate, fp.no_tile_filter, fp.n_slices])
    return sha(np.frombuffer(conf.encode(), np.uint8), fp.sao, fp.alf, t.slice_idx, t.col_bd, t.row_bd, *fp.aps, *(fp.planes if planes else []))


def stage_digests(out, stages, tables=()):
    """{key: sha256} of a run: one per output table, one per plane after each stage ("v0", "h2", "sao1", ...)."""
    rec = {n: sha(out[n]) for n in tables}
    for s in stages:
        rec.update({f"{s}{c}": sha(p) for c, p in enumerate(out[s])})
    return rec


def picture_names():
    return DEBLOCK + FILTER + [CHAIN]


def picture_digests(orc, name, run_d, run_f, run_c):
    """The record of tests/golden/ref_passes.json for one listed picture, computed by the given runs (run_d(pic), run_f(fp, stage), run_c())."""
    if name == CHAIN:
        d, fp = chain_picture()
        rec = {"inputs": sha(np.frombuffer((deblock_inputs_digest(d) + filter_inputs_digest(fp, False)).encode(), np.uint8))}
        rec.update(stage_digests(run_c(), ("v", "h", "sao", "alf"), d.t.OUT))
    elif name in DEBLOCK:
        pic = deblock_picture(orc, name)
        rec = {"inputs": deblock_inputs_digest(pic)}
        rec.update(stage_digests(run_d(pic), ("v", "h"), pic.t.OUT))
    else:
        fp = filter_picture(name)
        rec = {"inputs": filter_inputs_digest(fp)}
        rec.update(stage_digests({s: run_f(fp, s) for s in ("sao", "alf")}, ("sao", "alf")))
    return rec


def host_digests(orc, lib, side, name):
    return picture_digests(orc, name, lambda pic: run_deblock(lib, side, pic), lambda fp, s: run_filter(lib, side, fp, s), lambda: run_chain(lib, side))


def load_golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)["pictures"]


# ---------------------------------------------------------------------------------------------------------------- reading a difference

def read_mask(pic, name):
    """Entries of the output table `name` that the reference's filter loops read (ff_vvc_deblock_vertical / _horizontal): luma at every 4-grid
    position with x > 0 (vertical pass) or y > 0 (horizontal pass), chroma on the 8 << shift grid.  Derived from those loops, never from outputs."""
    t = pic.t
    d = int(name[2]) if name.startswith("bs") else int(name[1])             # 1 = vertical edges
    c = int(name[3]) if name.startswith("bs") else 0
    pos = 4 * (np.arange(t.tw) if d else np.arange(t.th))
    grid = 4 if c == 0 else 8 << (t.hs if d else t.vs)
    on = (pos > 0) & (pos % grid == 0)
    if c and pic.n_comp < 3:
        on[:] = False
    return np.broadcast_to(on[None, :] if d else on[:, None], (t.th, t.tw))


def table_differences(pic, want, got, names=None, label="reference"):
    """One line per differing output table: the first unit, both values, and whether the reference's filter loops read that entry."""
    lines = []
    for n in names or pic.t.OUT:
        bad = np.argwhere(want[n] != got[n])
        if len(bad):
            mask = read_mask(pic, n)
            read = [tuple(b) for b in bad if mask[tuple(b)]]
            b = read[0] if read else tuple(bad[0])
            lines.append(f"{pic.name} {n}: {len(bad)} entries differ ({len(read)} of them read by the filter loops), first at unit (row, col) "
                         f"{list(map(int, b))} = luma ({4 * b[1]}, {4 * b[0]}): {label} {want[n][b]}, other side {got[n][b]}, "
                         f"{'READ' if mask[b] else 'not read'} by the reference's filter loops")
    return lines


def plane_differences(name, stage, want, got, label="reference"):
    lines = []
    for c, (x, y) in enumerate(zip(want, got)):
        bad = np.argwhere(x != y)
        if len(bad):
            b = tuple(bad[0])
            lines.append(f"{name} after {stage}: component {c}: {len(bad)} samples differ, first at (row, col) {list(map(int, b))}: {label} {x[b]}, other side {y[b]}")
    return lines

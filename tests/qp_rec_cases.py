"""Pictures, sidecars, frames and expectations for vvc355_deblock_qp_rec_pass (the deblocking QP tables straight from the unit records):
the bs_rec_cases pictures with seeded QP sidecars, directed single-CTU pictures, the table setters' definition restated in numpy
(set_qp_y -> set_cb_tab over the coding unit, set_qp_c_tab -> set_tb_tab over the chroma transform block: vvc_ctu.c:144-185), the frame
builder, the device run, and the end-to-end deblocking case on the host.  Used by the tests and tools/deblock_qp_rec_time.py."""
import ctypes
from types import SimpleNamespace

import numpy as np

import bipred_cases as bc
import bs_rec_cases as rc
from ffvvc_amd import abi, batch

SEED = 0x5EED0C90
BD = 10
QP_BD_OFFSET = 6 * (BD - 8)
E2E = (1, 6)                                  # bs_rec_cases.CASES: 272x200 CTU 128 at 4:2:0, and the 4:2:2 picture
REC_DT = np.dtype(abi.CuRec, align=True)
TABLES = ("qp_y", "qp_c0", "qp_c1")


class Pic(SimpleNamespace):
    """A picture's records grouped per CTU with their sidecars: cu / tu (records), cu_first / tu_first (int32 ranges), cu_qp (int8[n_cu]),
    tu_qp_c (int8[n_tu][2]) and the geometry `g` (width, height, ctb_log2, cw, ch, tw, th: a BsTables has them all)."""


def geometry(width, height, ctb_log2):
    ctb = 1 << ctb_log2
    return SimpleNamespace(width=width, height=height, ctb_log2=ctb_log2, cw=(width + ctb - 1) // ctb, ch=(height + ctb - 1) // ctb,
                           tw=width // 4, th=height // 4)


def sidecars(rng, n_cu, n_tu):
    """QpY in [-qp_bd_offset, 63]; chroma pairs in [0, 63 + qp_bd_offset], drawn independently (Cb != Cr for most units)."""
    return (rng.integers(-QP_BD_OFFSET, 64, size=n_cu).astype(np.int8), rng.integers(0, 64 + QP_BD_OFFSET, size=(n_tu, 2)).astype(np.int8))


_pics = {}


def picture(orc, i):
    """bs_rec_cases' picture i (len(CASES) = BIG) with sidecars seeded by SEED + i; made once per process, nobody writes to it."""
    if i not in _pics:
        t, _ = rc.case(orc, i)
        (cu, cu_first), (tu, tu_first), _mv = rc.grouped(t)
        cu_qp, tu_qp_c = sidecars(np.random.default_rng(SEED + i), len(cu), len(tu))
        _pics[i] = Pic(g=t, cu=cu, tu=tu, cu_first=cu_first, tu_first=tu_first, cu_qp=cu_qp, tu_qp_c=tu_qp_c)
    return _pics[i]


def single_ctu(cu, tu, seed):
    """A 128x128 picture of one CTU from lists of (x0, y0, w, h, flags)."""
    cu = np.array([r + (0,) for r in cu], REC_DT)
    tu = np.array([r + (0,) for r in tu], REC_DT)
    cu_qp, tu_qp_c = sidecars(np.random.default_rng(SEED + seed), len(cu), len(tu))
    first = lambda n: np.array([0, n], np.int32)          # noqa: E731
    return Pic(g=geometry(128, 128, 7), cu=cu, tu=tu, cu_first=first(len(cu)), tu_first=first(len(tu)), cu_qp=cu_qp, tu_qp_c=tu_qp_c)


def directed(name):
    if name == "one_unit":                    # w = h = 128 in a uint8
        return single_ctu([(0, 0, 128, 128, 0)], [(0, 0, 128, 128, 0x01), (0, 0, 128, 128, 0x80)], 200)
    if name == "all_4x4":                     # 1024 + (1024 tree 0, then 1024 tree 1): the tree-1 records fill the second chunk of heads
        units = [(x, y, 4, 4) for y in range(0, 128, 4) for x in range(0, 128, 4)]
        return single_ctu([u + (0,) for u in units], [u + (0x01,) for u in units] + [u + (0x80,) for u in units], 201)
    if name == "odd_widths":                  # 3, 6 and 12 units wide: the paint path that keeps the division; the rest of the CTU stays uncovered
        cu = [(0, 0, 12, 8, 0), (12, 0, 24, 16, 0), (36, 0, 48, 32, 0), (84, 0, 44, 12, 0), (0, 64, 48, 12, 0), (48, 64, 24, 64, 0)]
        t1 = [(4, 8, 12, 12, 0x80), (16, 8, 24, 8, 0x82), (40, 8, 48, 24, 0x84), (88, 8, 40, 4, 0x80), (8, 80, 24, 48, 0x80), (80, 64, 48, 60, 0x86)]
        return single_ctu(cu, [(0, 0, 64, 64, 0x01)] + t1, 202)
    raise KeyError(name)


DIRECTED = ("one_unit", "all_4x4", "odd_widths")


def split(p):
    """Per CTU: [cu, cu_qp, tu, tu_qp_c] (copies), to be edited and handed to join()."""
    out = []
    for rs in range(p.g.cw * p.g.ch):
        c, u = slice(p.cu_first[rs], p.cu_first[rs + 1]), slice(p.tu_first[rs], p.tu_first[rs + 1])
        out.append([p.cu[c].copy(), p.cu_qp[c].copy(), p.tu[u].copy(), p.tu_qp_c[u].copy()])
    return out


def join(g, ctus):
    """The picture of per-CTU lists as split() makes them: records stay filed under the CTU whose list holds them."""
    first = lambda k: np.concatenate([[0], np.cumsum([len(c[k]) for c in ctus])]).astype(np.int32)          # noqa: E731
    cat = lambda k: np.concatenate([c[k] for c in ctus])                                                      # noqa: E731
    return Pic(g=g, cu=cat(0), cu_qp=cat(1), tu=cat(2), tu_qp_c=cat(3), cu_first=first(0), tu_first=first(2))


def paints(g, recs, first):
    """The records that paint: positive sizes, everything a multiple of 4, the rectangle inside the CTU the record is FILED under."""
    x0, y0, w, h = (recs[k].astype(np.int64) for k in ("x0", "y0", "w", "h"))
    rs = np.searchsorted(first, np.arange(len(recs)), side="right") - 1
    ox, oy, ctb = (rs % g.cw) << g.ctb_log2, (rs // g.cw) << g.ctb_log2, 1 << g.ctb_log2
    ok = (w > 0) & (h > 0) & (((w | h | x0 | y0) & 3) == 0)
    return ok & (x0 >= ox) & (y0 >= oy) & (x0 + w <= ox + ctb) & (y0 + h <= oy + ctb)


def paint(g, recs, first, values, keep=None):
    """expected = zeros; for each well-formed record: table[rect] = value (the part inside the picture)."""
    tab = np.zeros((g.th, g.tw), np.int8)
    ok = paints(g, recs, first) & (True if keep is None else keep)
    for r, v in zip(recs[ok], values[ok]):
        tab[r["y0"] // 4:(int(r["y0"]) + int(r["h"])) // 4, r["x0"] // 4:(int(r["x0"]) + int(r["w"])) // 4] = v
    return tab


def expected(p):
    """{qp_y, qp_c0, qp_c1} of the picture: coding units paint qp_y, tree-1 transform units paint qp_c."""
    tree1 = (p.tu["flags"] & 0x80) != 0
    return {"qp_y": paint(p.g, p.cu, p.cu_first, p.cu_qp),
            "qp_c0": paint(p.g, p.tu, p.tu_first, p.tu_qp_c[:, 0], tree1), "qp_c1": paint(p.g, p.tu, p.tu_first, p.tu_qp_c[:, 1], tree1)}


def aligned_pitch(g):
    return (g.tw + 7) // 4 * 4                # > tw, every row starts on a dword


def odd_pitch(g):
    return (g.tw + 4) | 1                     # > tw, three rows out of four start off a dword


def qp_frame(g, cu, tu, cu_qp, tu_qp_c, outs, pitch, n_comp=3):
    """abi.QpRecFrame: cu / tu = (device address, count, device address of ctu_first); outs = device addresses of qp_y, qp_c[0], qp_c[1]."""
    f = abi.QpRecFrame()
    f.cu, f.n_cu, f.ctu_first_cu = cu
    f.tu, f.n_tu, f.ctu_first_tu = tu
    f.cu_qp, f.tu_qp_c = cu_qp, tu_qp_c
    f.qp_y, f.qp_c[0], f.qp_c[1] = outs
    f.unit_pitch, f.width, f.height, f.ctb_width, f.ctb_height = pitch, g.width, g.height, g.cw, g.ch
    f.ctb_log2, f.n_comp = g.ctb_log2, n_comp
    return f


def upload(a):
    return batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a) if len(a) else None


def run_device(dev, p, pitch=None, n_comp=3, with_tu=True):
    """vvc355_deblock_qp_rec_pass on outputs pre-filled with 0xEE: {name: int8 (th, pitch)}, the pitch padding included.  with_tu = False:
    tu, ctu_first_tu, tu_qp_c and qp_c are passed as 0 (n_comp = 1)."""
    g = p.g
    pitch = pitch or aligned_pitch(g)
    outs = {name: batch.DeviceBuffer.from_host(np.full((g.th, pitch), 0xEE, np.uint8)) for name in TABLES}
    d = [upload(a) for a in (p.cu, p.cu_first, p.cu_qp)] + [upload(a) if with_tu else None for a in (p.tu, p.tu_first, p.tu_qp_c)]
    a = [b.ptr if b else 0 for b in d]
    f = qp_frame(g, (a[0], len(p.cu), a[1]), (a[3], len(p.tu) if with_tu else 0, a[4]), a[2], a[5],
                 [outs[n].ptr if with_tu or n == "qp_y" else 0 for n in TABLES], pitch, n_comp)
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    err = dev.vvc355_deblock_qp_rec_pass(None, d_f.ptr, ctypes.addressof(f))
    assert err == 0, f"vvc355_deblock_qp_rec_pass refused the frame: {err}"
    dev.vvc355_stream_sync(None)
    return {name: outs[name].to_host(np.int8, (g.th, pitch)) for name in TABLES}


def mismatches(got, want, g, names=TABLES):
    """One line per table that differs inside the picture or whose pitch padding lost its sentinel."""
    lines = []
    for name in names:
        bad = np.argwhere(got[name][:, :g.tw] != want[name])
        if len(bad):
            b = tuple(bad[0])
            lines.append(f"{name}: {len(bad)} entries differ, first at (row, col) {list(b)}: got {got[name][b]}, want {want[name][b]}")
        pad = got[name][:, g.tw:].view(np.uint8)
        if np.any(pad != 0xEE):
            lines.append(f"{name}: {int(np.count_nonzero(pad != 0xEE))} entries of the pitch padding were written")
    return lines


# ---- end to end: the deblocking passes on the oracle's bS tables and the painter's QP tables

_e2e = {}


def e2e_inputs(orc, i):
    """Case i at 10 bit: (planes, dims, db_params) as test_chain_gpu.py makes them; made once, nobody writes to them."""
    if i not in _e2e:
        t, _ = rc.case(orc, i)
        rng = np.random.default_rng(SEED + 300 + i)
        dims = [(t.width, t.height)] + [(t.width >> t.hs, t.height >> t.vs)] * 2
        planes = []
        for (pw, ph) in dims:
            base = bc.smooth_picture(rng, ph, pw, BD, scale=32).astype(np.int64)
            offs = rng.integers(-(1 << (BD - 6)), (1 << (BD - 6)) + 1, size=(ph // 4, pw // 4))
            planes.append(np.clip(base + np.kron(offs, np.ones((4, 4), np.int64)), 0, (1 << BD) - 1).astype(np.uint16))
        _e2e[i] = (planes, dims, rng.integers(-7, 8, size=(t.cw * t.ch, 6)).astype(np.int8))
    return _e2e[i]


def deblock_frame(t, vertical, planes, strides, tab, qp, dbp):
    """abi.DeblockFrame of one pass: tab(name) = address of the bS / length / tb_size table `name` (BsTables names), qp = addresses of
    qp_y, qp_c[0], qp_c[1]; every table with row pitch t.tw, minimum coding block 4."""
    f = abi.DeblockFrame()
    for c in range(3):
        f.plane[c], f.stride[c], f.bs[c] = planes[c], strides[c], tab(f"bs{vertical}{c}")
    f.max_len_p, f.max_len_q, f.tb_size_c = tab(f"p{vertical}"), tab(f"q{vertical}"), tab("tbw1" if vertical else "tbh1")
    f.qp_y, f.qp_c[0], f.qp_c[1], f.db_params = qp[0], qp[1], qp[2], dbp
    f.width, f.height, f.min_tu_width, f.min_cb_width, f.ctb_width = t.width, t.height, t.tw, t.tw, t.cw
    f.min_cb_log2, f.ctb_log2, f.hs, f.vs, f.n_comp, f.vertical = 2, t.ctb_log2, t.hs, t.vs, 3, vertical
    f.qp_bd_offset = QP_BD_OFFSET
    return f


def e2e_oracle(orc, i, qp):
    """orc_deblock_frame_pass, vertical then horizontal, on copies of case i's planes with the oracle's bS tables and the QP tables `qp`
    ({qp_y, qp_c0, qp_c1}, int8 (th, tw)): the deblocked planes."""
    orc.orc_deblock_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.DeblockFrame)]
    orc.orc_deblock_frame_pass.restype = None
    t, want = rc.case(orc, i)
    planes, dims, dbp = e2e_inputs(orc, i)
    out = [p.copy() for p in planes]
    tabs = {**want, "tbw1": t.tbw1, "tbh1": t.tbh1}
    q = [np.ascontiguousarray(qp[n]) for n in TABLES]
    for vertical in (1, 0):
        f = deblock_frame(t, vertical, [p.ctypes.data for p in out], [d[0] * 2 for d in dims], lambda n: tabs[n].ctypes.data,
                          [a.ctypes.data for a in q], dbp.ctypes.data)
        orc.orc_deblock_frame_pass(BD, ctypes.byref(f))
    return out

"""Pictures, frames and expectations for vvc355_deblock_bs_rec_pass (boundary strengths straight from the unit records): the case list of
the CPU and GPU tests, the frame built from a bs_cases.BsTables and its grouped records, the device run (motion-only table fill, then the
pass) and the completeness rule of the header restated in numpy for pictures with holes.  Used by the tests and tools/deblock_bs_rec_time.py."""
import ctypes

import numpy as np

import bs_cases
from ffvvc_amd import abi, batch

SEED = 0x5EED0B70
CASES = [
    dict(width=72, height=40, ctb_log2=7),                                                          # a single partial CTU, no halo
    dict(width=272, height=200, ctb_log2=7),                                                        # 3 x 2 CTUs, partial right and bottom
    dict(width=328, height=200, ctb_log2=6, n_slices=3, tiles=True, lfase=0, lfate=0),
    dict(width=416, height=240, ctb_log2=7, n_slices=4, tiles=True, lfase=1, lfate=0),
    dict(width=416, height=240, ctb_log2=7, n_slices=4, tiles=True, lfase=0, lfate=1),
    dict(width=264, height=136, ctb_log2=5, n_slices=5, tiles=True, lfase=0, lfate=0),
    dict(width=328, height=200, ctb_log2=6, n_slices=3, tiles=True, lfase=0, lfate=0, hs=1, vs=0),  # case 2's geometry at 4:2:2
    dict(width=328, height=200, ctb_log2=6, n_slices=2, hs=0, vs=0),                                # 4:4:4
]
BIG = dict(width=1480, height=840, ctb_log2=7)              # against the table path on the device; seed SEED + len(CASES)
OUT_C = ("bs01", "bs02", "bs11", "bs12")                    # the chroma outputs among BsTables.OUT
TB_C = ("tbw1", "tbh1")                                     # tb_width_c / tb_height_c: what the generator filled unit by unit

_cache = {}


def case(orc, i):
    """(tables, oracle outputs) of case i (len(CASES) = BIG), made once per process; nobody writes to either."""
    if i not in _cache:
        t = bs_cases.BsTables(np.random.default_rng(SEED + i), **(CASES[i] if i < len(CASES) else BIG))
        _cache[i] = (t, bs_cases.run_oracle(orc, t))
    return _cache[i]


def grouped(t, recs=None):
    """[(records, ctu_first)] for cu, tu, mv: per CTU in raster order, as both record passes take them."""
    return [t.group_per_ctu(r, t.ctb_log2, t.cw, t.cw * t.ch) for r in (recs if recs is not None else t.records())]


def rec_frame(t, cu, tu, ptr_of, n_comp=3, tb_c=True):
    """abi.BsRecFrame of picture `t`: cu / tu = (device address, count, device address of ctu_first); ptr_of(name) = device address of the
    table `name` (BsTables names; tb_width_c / tb_height_c are "tbw1" / "tbh1")."""
    f = abi.BsRecFrame()
    f.cu, f.n_cu, f.ctu_first_cu = cu
    f.tu, f.n_tu, f.ctu_first_tu = tu
    f.mvf, f.ref_poc, f.slice_idx = ptr_of("mvf"), ptr_of("ref_poc"), ptr_of("slice_idx")
    f.ctb_to_col_bd, f.ctb_to_row_bd = ptr_of("col_bd"), ptr_of("row_bd")
    for d in range(2):
        for c in range(3 if n_comp == 3 else 1):
            f.bs[d][c] = ptr_of(f"bs{d}{c}")
        f.max_len_p[d], f.max_len_q[d] = ptr_of(f"p{d}"), ptr_of(f"q{d}")
    if tb_c:
        f.tb_width_c, f.tb_height_c = ptr_of("tbw1"), ptr_of("tbh1")
    f.unit_pitch = f.mvf_pitch = t.tw
    f.width, f.height, f.ctb_width, f.ctb_height = t.width, t.height, t.cw, t.ch
    f.ctb_log2, f.hs, f.vs, f.n_comp, f.lfase, f.lfate = t.ctb_log2, t.hs, t.vs, n_comp, t.lfase, t.lfate
    return f


def fill_mvf(dev, t, mv, mv_first, d_mvf, stream=None, keep=None):
    """The MvField table from the motion records alone: vvc355_tab_fill_pass with n_cu = n_tu = 0."""
    d_mv, d_first = batch.DeviceBuffer.from_host(mv.view(np.uint8)), batch.DeviceBuffer.from_host(mv_first)
    f = t.fill_frame(0, 0, d_mv.ptr, (0, 0, len(mv)), lambda name: d_mvf.ptr if name == "mvf" else 0, (0, 0, d_first.ptr))
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    dev.vvc355_tab_fill_pass(stream, d_f.ptr, ctypes.addressof(f))
    if keep is not None:
        keep += [d_mv, d_first, d_f, f]
    else:
        dev.vvc355_stream_sync(stream)


def run_device(dev, t, groups, n_comp=3, tb_c=True):
    """Motion-only fill, then vvc355_deblock_bs_rec_pass on outputs pre-filled with 0xEE: {name: table} for BsTables.OUT + TB_C."""
    (cu, cu_first), (tu, tu_first), (mv, mv_first) = groups
    sentinel = np.full((t.th, t.tw), 0xEE, np.uint8)
    bufs = {name: batch.DeviceBuffer.from_host(sentinel) for name in t.OUT + TB_C}
    bufs["mvf"] = batch.DeviceBuffer(t.mvf.nbytes)
    for name in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
        bufs[name] = batch.DeviceBuffer.from_host(getattr(t, name))
    fill_mvf(dev, t, mv, mv_first, bufs["mvf"])
    d = [batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a) if len(a) else None for a in (cu, cu_first, tu, tu_first)]
    p = [b.ptr if b else 0 for b in d]
    f = rec_frame(t, (p[0], len(cu), p[1]), (p[2], len(tu), p[3]), lambda name: bufs[name].ptr, n_comp, tb_c)
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    rc = dev.vvc355_deblock_bs_rec_pass(None, d_f.ptr, ctypes.addressof(f))
    assert rc == 0, f"vvc355_deblock_bs_rec_pass refused the frame: {rc}"
    dev.vvc355_stream_sync(None)
    return {name: bufs[name].to_host(np.uint8, (t.th, t.tw)) for name in t.OUT + TB_C}


def mismatches(got, want, names):
    """One line per table that differs, with the first position, as test_deblock_bs_gpu.py reports them."""
    lines = []
    for name in names:
        bad = np.argwhere(got[name] != want[name])
        if len(bad):
            b = tuple(bad[0])
            lines.append(f"{name}: {len(bad)} entries differ, first at (row, col) {list(b)}: got {got[name][b]}, want {want[name][b]}")
    return lines


def expected(t, want):
    """The oracle's outputs plus tb_*_c of a picture whose records cover it."""
    return {**want, "tbw1": t.tbw1, "tbh1": t.tbh1}


def ctu_starts(t, axis):
    """Unit columns (axis 1) / rows (axis 0) that start a CTU, the picture's first left out."""
    per, n = 1 << (t.ctb_log2 - 2), t.tw if axis else t.th
    return np.arange(per, n, per)


def well_formed(t, recs):
    """The records that the pass paints: positive sizes, everything a multiple of 4, the rectangle inside the CTU of its origin."""
    x0, y0, w, h = (recs[k].astype(np.int64) for k in ("x0", "y0", "w", "h"))
    ctb = 1 << t.ctb_log2
    ok = (w > 0) & (h > 0) & (((w | h | x0 | y0) & 3) == 0) & (x0 >= 0) & (y0 >= 0)
    return ok & ((x0 & (ctb - 1)) + w <= ctb) & ((y0 & (ctb - 1)) + h <= ctb)


def coverage(t, recs, keep):
    """Units (th x tw, bool) that a record of `recs[keep]` covers."""
    m = np.zeros((t.th, t.tw), bool)
    for r in recs[keep & well_formed(t, recs)]:
        m[r["y0"] // 4:(int(r["y0"]) + int(r["h"])) // 4, r["x0"] // 4:(int(r["x0"]) + int(r["w"])) // 4] = True
    return m


def expected_with_holes(t, want, cu, tu, n_comp=3):
    """The completeness rule of include/vvc_mi355.h on the oracle's outputs of the FULL picture: a unit is complete with a coding-unit, a
    tree-0 and (n_comp == 3) a tree-1 record; the entries of (unit, direction) are 0 where the unit or its P side is not.  Returns
    (tables, zeroed[2] masks).  (The generator's transform units lie inside their coding units, so the coding unit at a transform unit's
    origin is missing only where the unit's own is.)"""
    tree1 = (tu["flags"] & 0x80) != 0
    has_t1 = coverage(t, tu, tree1)
    complete = coverage(t, cu, np.ones(len(cu), bool)) & coverage(t, tu, ~tree1) & (has_t1 if n_comp == 3 else True)
    zeroed = [~complete, ~complete]
    zeroed[0] = zeroed[0].copy()
    zeroed[1] = zeroed[1].copy()
    zeroed[0][1:, :] |= ~complete[:-1, :]            # dir 0: the P side is the unit above
    zeroed[1][:, 1:] |= ~complete[:, :-1]            # dir 1: the unit to the left
    out = {}
    for name in t.OUT:
        d = int(name[2]) if name.startswith("bs") else int(name[1])
        out[name] = np.where(zeroed[d], 0, want[name]).astype(np.uint8)
    out["tbw1"], out["tbh1"] = np.where(has_t1, t.tbw1, 0).astype(np.uint8), np.where(has_t1, t.tbh1, 0).astype(np.uint8)
    return out, zeroed

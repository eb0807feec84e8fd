"""The picture pass of the deblocking filter (vvc355_deblock_frame_pass) with its samples held two lines per register: whole small
pictures, vertical pass then horizontal pass, compared sample for sample with orc_deblock_frame_pass on the same tables.

The pictures are built so that every filter class occurs, and the oracle's own output is asked to prove it before anything is
compared (test_oracle_* need no GPU).  Across the edges a picture has three zones: edges 16 apart (every length pair of
{1, 2, 3, 5, 7}^2), 8 apart (pairs of {1, 2, 3}^2), and the 4-grid (length 1); the edge between two zones takes the lengths of the
narrower one.  The height puts a CTU-row edge (ctb_log2 = 5) into the 16-zone, where the horizontal pass cuts luma len_p to 3 and
chroma len_p to 1."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import P, load_oracle, px_dtype
from ffvvc_amd import abi, batch
from test_deblock_frame_gpu import side_tables

FMT = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
LONG = [(a, b) for a in (1, 2, 3, 5, 7) for b in (1, 2, 3, 5, 7)]
SHORT = [(a, b) for a in (1, 2, 3) for b in (1, 2, 3)]


def zones(n):
    """(end of the 16-zone, end of the 8-zone) across an axis of n samples."""
    a = 16 * ((n - 24) // 16)
    return a, a + 16


def spacing(n, pos):
    """Distance to the next edge on the narrower side of the edge at pos."""
    a, b = zones(n)
    return 16 if pos < a else 8 if pos < b else 4


def is_edge(n, pos):
    a, b = zones(n)
    return pos % (16 if pos <= a else 8 if pos <= b else 4) == 0


def zone_tables(rng, w, h, vertical, shift, p_zero=0.1):
    """bs[3], len_p, len_q, tb_size_c of one pass, per 4x4 luma unit, laid out in the zones above."""
    tw, th = w // 4, h // 4
    bs = np.zeros((3, th, tw), np.uint8)
    len_p, len_q = np.zeros((th, tw), np.uint8), np.zeros((th, tw), np.uint8)
    tb_c = np.full((th, tw), 4, np.uint8)
    n_across, n_along = (w, th) if vertical else (h, tw)
    a_end, _ = zones(n_across)
    count = [0, 0]
    for pos in range(4, n_across, 4):
        if not is_edge(n_across, pos):
            continue
        sp = spacing(n_across, pos)
        for k in range(n_along):
            y, x = (k, pos // 4) if vertical else (pos // 4, k)
            bs[0, y, x] = rng.choice([0, 1, 2], p=[p_zero, (1 - p_zero) / 2, (1 - p_zero) / 2])
            if sp == 16:
                len_p[y, x], len_q[y, x] = LONG[count[0] % 25]
                count[0] += 1
            elif sp == 8:
                len_p[y, x], len_q[y, x] = SHORT[count[1] % 9]
                count[1] += 1
            else:
                len_p[y, x] = len_q[y, x] = 1
            if pos % (8 << shift) == 0:
                bs[1, y, x] = rng.choice([0, 1, 2], p=[p_zero, (1 - p_zero) / 2, (1 - p_zero) / 2])
                bs[2, y, x] = rng.choice([0, 1, 2], p=[p_zero, (1 - p_zero) / 2, (1 - p_zero) / 2])
    # chroma transform sizes: 8 or more on both sides of the 16-zone's edges (the three-tap chroma filters), 4 elsewhere
    if vertical:
        tb_c[:, :a_end // 4] = 16
    else:
        tb_c[:a_end // 4, :] = 16
    return bs, len_p, len_q, tb_c


def grid4_tables(rng, w, h, vertical, shift):
    """A partition that is 4 wide everywhere: bs != 0 on every edge of the 4-grid (chroma: of its 8-grid), length 1."""
    tw, th = w // 4, h // 4
    bs = np.zeros((3, th, tw), np.uint8)
    for pos in range(1, tw if vertical else th):
        sel = (slice(None), pos) if vertical else (pos, slice(None))
        n = th if vertical else tw
        bs[0][sel] = rng.integers(1, 3, size=n)
        if (pos * 4) % (8 << shift) == 0:
            bs[1][sel] = rng.integers(1, 3, size=n)
            bs[2][sel] = rng.integers(1, 3, size=n)
    ones = np.ones((th, tw), np.uint8)
    return bs, ones, ones.copy(), np.full((th, tw), 2 if shift else 4, np.uint8)


def cells(w, h):
    """Cell number of every sample for cells as wide / tall as the zone they are in (so that cell borders are the zones' edges)."""
    def axis(n):
        idx, pos, k = np.zeros(n, np.int64), 0, 0
        while pos < n:
            s = spacing(n, pos) if pos else 16
            idx[pos:pos + s] = k
            pos, k = pos + s, k + 1
        return idx
    return axis(w)[None, :], axis(h)[:, None]


def content(rng, kind, pw, ph, bd, sub):
    """One plane.  sub = (hs, vs): the luma zones are laid over the plane at its own scale."""
    top = (1 << bd) - 1
    sc = 1 << (bd - 8)
    cx, cy = cells(pw << sub[0], ph << sub[1])
    cx, cy = cx[:, ::1 << sub[0]], cy[::1 << sub[1], :]
    xx, yy = np.meshgrid(np.arange(pw), np.arange(ph))
    if kind == "flat":                          # flat cells, a step of 4..6 between them (8-bit units: the third tap of the strong filter
        # moves by (step + 4) >> 3; tc is 6 or more at the QPs used)
        step = rng.integers(4, 7, size=(int(cy.max()) + 1, int(cx.max()) + 1)) * sc
        v = 100 * sc + step[cy, cx] * ((cx + cy) & 1)
    elif kind == "ramp":                        # slopes too steep for the strong / long decisions, a small step per cell and noise
        tri = 64 - np.abs((xx + yy) % 128 - 64)                                  # up and down, so that the ramp stays in range
        v = 30 * sc + (3 * sc) * tri + (2 * sc) * ((cx + cy) & 1) + rng.integers(-1, 2, size=(ph, pw)) * max(1, sc // 2)
    elif kind == "noise":
        v = rng.integers(0, top + 1, size=(ph, pw))
    elif kind == "max":
        v = np.full((ph, pw), top)
    elif kind.startswith("cols"):
        v = ((xx // int(kind[4:])) & 1) * top
    elif kind.startswith("rows"):
        v = ((yy // int(kind[4:])) & 1) * top
    else:
        raise ValueError(kind)
    return np.clip(v, 0, top).astype(px_dtype(bd))


class Case:
    """One picture: planes before, the per-pass tables, and the oracle's planes after each pass (computed once)."""

    def __init__(self, kind, bd, fmt, w=136, h=72, ctb_log2=5, tables="zones", qp="mid", seed=0):
        self.kind, self.bd, self.fmt, self.w, self.h, self.ctb_log2 = kind, bd, fmt, w, h, ctb_log2
        hs, vs = self.hs, self.vs = FMT[fmt]
        rng = np.random.default_rng([0x5EED0D8, seed, bd, hs, vs, w, h])
        self.dims = [(w, h), (w >> hs, h >> vs), (w >> hs, h >> vs)]
        self.planes = [content(rng, kind, pw, ph, bd, (hs, vs) if c else (0, 0)) for c, (pw, ph) in enumerate(self.dims)]
        tw, th = w // 4, h // 4
        self.ctb_w, self.ctb_h = -(-w >> ctb_log2), -(-h >> ctb_log2)
        self.cb_w = -(-w // 8)
        bdo = 6 * (bd - 8)
        # mid: QPs where beta and tc are large enough for every decision to go both ways; top: the last entries of Table 43
        # (tc' = 395, beta' = 88); zero: tc' = 0 everywhere
        q = {"mid": (34, 42), "top": (63, 64), "zero": (4, 11)}[qp]
        self.qp_y = rng.integers(q[0], q[1], size=(-(-h // 8), self.cb_w)).astype(np.int8)
        self.qp_c = [(rng.integers(q[0], q[1], size=(th, tw)) + bdo).astype(np.int8) for _ in range(2)]
        n_ctb = self.ctb_w * self.ctb_h
        self.dbp = {"mid": rng.integers(-4, 5, size=(n_ctb, 6)), "top": np.full((n_ctb, 6), 12), "zero": np.zeros((n_ctb, 6))}[qp].astype(np.int8)
        self.ladf = qp == "mid"
        self.tabs = {}
        for vertical in (1, 0):
            shift = hs if vertical else vs
            if tables == "zones":
                t = zone_tables(rng, w, h, vertical, shift)
            elif tables == "grid4":
                t = grid4_tables(rng, w, h, vertical, shift)
            elif tables == "bs0":
                t = zone_tables(rng, w, h, vertical, shift, p_zero=1.0)
            else:                               # the random partition of test_deblock_frame_gpu.py, which is made of 32x32 blocks: the
                # block that the picture border cuts across the edges becomes 4 wide, as a decoder's implicit split would leave it
                tsize, bs, lp, lq = side_tables(rng, -(-w // 32) * 32, -(-h // 32) * 32, vertical, shift)
                tsize, bs, lp, lq = tsize[:th, :tw], bs[:, :th, :tw], lp[:th, :tw], lq[:th, :tw]
                cut = (w if vertical else h) // 32 * 8
                sel = (slice(None), slice(cut, None)) if vertical else (slice(cut, None), slice(None))
                tsize[sel], lp[sel], lq[sel] = 4, np.minimum(lp[sel], 1), np.minimum(lq[sel], 1)
                t = (bs, lp, lq, np.maximum(tsize >> shift, 2).astype(np.uint8))
            self.tabs[vertical] = [np.ascontiguousarray(a) for a in (t[0][0], t[0][1], t[0][2], t[1], t[2], t[3], self.qp_y, self.qp_c[0], self.qp_c[1], self.dbp)]
        self.after = {}
        self.isz = 1 if bd == 8 else 2

    def fill(self, f, planes_ptr, strides, tabs, vertical):
        for c in range(3):
            f.plane[c], f.stride[c], f.bs[c] = planes_ptr[c], strides[c], tabs[c]
        f.max_len_p, f.max_len_q, f.tb_size_c, f.qp_y = tabs[3], tabs[4], tabs[5], tabs[6]
        f.qp_c[0], f.qp_c[1], f.db_params = tabs[7], tabs[8], tabs[9]
        f.width, f.height, f.min_tu_width, f.min_cb_width, f.ctb_width = self.w, self.h, self.w // 4, self.cb_w, self.ctb_w
        f.min_cb_log2, f.ctb_log2, f.hs, f.vs, f.n_comp, f.vertical = 3, self.ctb_log2, self.hs, self.vs, 3, vertical
        f.qp_bd_offset = 6 * (self.bd - 8)
        f.ladf_enabled, f.num_ladf_intervals, f.ladf_lowest_qp_offset = int(self.ladf), 4, -3
        for k, v in enumerate((2, -1, 4, 0)):
            f.ladf_qp_offset[k] = v
        for k, v in enumerate((0, 1 << (self.bd - 3), 1 << (self.bd - 2), 1 << (self.bd - 1), 0)):
            f.ladf_lower_bound[k] = v

    def oracle(self, orc):
        """The planes after the vertical pass (key 1) and after both (key 0)."""
        if not self.after:
            orc.orc_deblock_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.DeblockFrame)]
            orc.orc_deblock_frame_pass.restype = None
            cur = [p.copy() for p in self.planes]
            for vertical in (1, 0):
                hf = abi.DeblockFrame()
                self.fill(hf, [P(p) for p in cur], [self.dims[c][0] * self.isz for c in range(3)], [P(t) for t in self.tabs[vertical]], vertical)
                orc.orc_deblock_frame_pass(self.bd, ctypes.byref(hf))
                self.after[vertical] = [p.copy() for p in cur]
                for p in self.after[vertical]:
                    p.setflags(write=False)
        return self.after

    def changed(self, orc, vertical, c=0):
        """Mask of the samples of component c the oracle changed in one pass, with the edges running down the columns (the horizontal
        pass transposed), so that axis 1 is the position across the edges."""
        after = self.oracle(orc)
        before = self.planes[c] if vertical else after[1][c]
        m = after[vertical][c] != before
        return m if vertical else m.T


@functools.lru_cache(maxsize=None)
def case(*a, **k):
    return Case(*a, **k)


def kw(**k):
    return tuple(sorted(k.items()))


def run_gpu(dev, orc, cs):
    want = cs.oracle(orc)
    pitched = [batch.to_pitched(p) for p in cs.planes]
    d_planes = [batch.DeviceBuffer.from_host(p) for p in pitched]
    for vertical in (1, 0):
        dev_tabs = [batch.DeviceBuffer.from_host(t) for t in cs.tabs[vertical]]
        df = abi.DeblockFrame()
        cs.fill(df, [d.ptr for d in d_planes], [pitched[c].shape[1] * cs.isz for c in range(3)], [d.ptr for d in dev_tabs], vertical)
        d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(df), np.uint8))
        dev.vvc355_deblock_frame_pass(None, cs.bd, d_f.ptr, ctypes.addressof(df))
        dev.vvc355_stream_sync(None)
        for c in range(3):
            got = d_planes[c].to_host(pitched[c].dtype, pitched[c].shape)[:, :cs.dims[c][0]]
            bad = np.argwhere(got != want[vertical][c])
            assert len(bad) == 0, (f"{cs.kind} bd={cs.bd} {cs.fmt} pass vertical={vertical} component {c}: {len(bad)} samples differ, "
                                   f"first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[vertical][c][tuple(bad[0])]}")


# ---------------------------------------------------------------- what the oracle did: every class occurred (no device code)

def zone_cols(n, lo, hi, period, phases):
    return [x for x in range(lo, hi) if x % period in phases and x < n]


def check_flat(cs, orc):
    """Flat cells with small steps: the long filters reach four or more samples from an edge of the 16-zone (but not on the p side of a
    CTU-row edge in the horizontal pass); the strong filter of the 8-zone changes the third sample and never the fourth."""
    for vertical in (1, 0):
        m = cs.changed(orc, vertical)
        n = m.shape[1]
        a, b = zones(n)
        assert m[:, zone_cols(n, 16, a, 16, range(4, 12))].any(), "no long filter fired"
        third, fourth = [a - 3, a + 2, a + 5, a + 10], [a - 4, a + 3, a + 4, a + 11]      # of the two length-3 edges, at a and a + 8
        assert m[:, third].any() and not m[:, fourth].any(), "8-zone: third sample unchanged, or fourth changed"
        assert not m[:, zone_cols(n, b + 4, n, 4, (1, 2))].any(), "4-grid: a sample other than p0 / q0 changed"
        if not vertical:
            for e in range(1 << cs.ctb_log2, a, 1 << cs.ctb_log2):
                assert not m[:, e - 8:e - 3].any() and m[:, e - 3:e].any() and m[:, e + 4:e + 7].any(), f"CTU-row edge {e}: len_p not cut to 3"
        # chroma: three taps on both sides in the 16-zone, one on the p side of a CTU-row edge
        hs, vs = (cs.hs, cs.vs) if vertical else (cs.vs, cs.hs)
        for c in (1, 2):
            mc = cs.changed(orc, vertical, c)
            g = 16 >> hs                                        # the chroma plane's edge spacing in the 16-zone
            cols = [x for x in range(g, a >> hs) if x % g in (2, g - 3)]
            assert mc[:, cols].any(), f"chroma {c}: no three-tap filter fired"
            if not vertical:
                for e in range(1 << cs.ctb_log2, a, 1 << cs.ctb_log2):
                    ec = e >> hs
                    assert not mc[:, ec - 3:ec - 1].any() and mc[:, ec + 1:ec + 3].any(), f"chroma {c} CTU-row edge {e}: len_p not cut to 1"


def check_ramp(cs, orc):
    """Steep ramps: the weak filter only, so nothing beyond the second sample of a side changes, and p1 / q1 change somewhere."""
    for vertical in (1, 0):
        m = cs.changed(orc, vertical)
        n = m.shape[1]
        a, b = zones(n)
        inner = zone_cols(n, 16, a, 16, range(2, 14)) + zone_cols(n, a + 8, b, 8, range(2, 6))
        assert not m[:, inner].any(), "a strong or long filter fired on the ramps"
        assert m[:, zone_cols(n, 16, a, 16, (0, 15))].any(), "no weak filter fired"
        assert m[:, zone_cols(n, 16, a, 16, (1, 14))].any(), "the weak filter never changed a second sample"


def check_noise(cs, orc):
    for vertical in (1, 0):
        m = cs.changed(orc, vertical)
        assert m.mean() < 0.03, f"{m.mean():.3f} of the noise picture's luma changed"


CLASS_CASES = [(k, bd, fmt) for k in ("flat", "ramp", "noise") for (bd, fmt) in ((8, "420"), (10, "420"), (12, "420"), (10, "422"), (10, "444"), (8, "444"))]
CHECK = {"flat": check_flat, "ramp": check_ramp, "noise": check_noise}


@pytest.mark.parametrize("kind,bd,fmt", CLASS_CASES)
def test_oracle_classes_occur(orc, kind, bd, fmt):
    CHECK[kind](case(kind, bd, fmt), orc)


def test_oracle_length_pairs_all_fed():
    cs = case("flat", 10, "420")
    for vertical in (1, 0):
        bs, lp, lq = cs.tabs[vertical][0], cs.tabs[vertical][3], cs.tabs[vertical][4]
        pairs = {(int(p), int(q)) for p, q, s in zip(lp.ravel(), lq.ravel(), bs.ravel()) if s}
        assert pairs >= set(LONG), f"vertical={vertical}: length pairs never fed: {sorted(set(LONG) - pairs)}"


def test_oracle_extremes_reach_the_filters(orc):
    """Blocks of 0 / max with tc = 395: the weak filter moves samples by the full tc; the all-max picture is left as it is."""
    cs = case("cols16", 10, "420", qp="top")
    after = cs.oracle(orc)
    d = np.abs(after[1][0].astype(np.int64) - cs.planes[0].astype(np.int64))
    assert d.max() >= 384, f"largest change {d.max()}"
    cs = case("max", 10, "420", qp="top")
    assert all(np.array_equal(a, b) for a, b in zip(cs.oracle(orc)[0], cs.planes))


HALF_UNIT = [(t, bd, fmt) for t in ("zones", "grid4", "random") for (bd, fmt) in ((8, "420"), (10, "420"), (10, "444"), (12, "420"))]


@pytest.mark.parametrize("tables,bd,fmt", HALF_UNIT)
def test_oracle_stays_inside_the_rows(orc, tables, bd, fmt):
    """The tables of the cut pictures are valid: no filter reaches past the end of a row (the oracle's result on planes with a wide,
    zeroed pitch is the one on contiguous planes; the device's planes are pitched)."""
    cs = case("flat", bd, fmt, w=132, h=68, tables=tables)
    want = cs.oracle(orc)
    wide = [np.zeros((p.shape[0] + 8, p.shape[1] + 64), p.dtype) for p in cs.planes]
    for a, p in zip(wide, cs.planes):
        a[:p.shape[0], :p.shape[1]] = p
    for vertical in (1, 0):
        hf = abi.DeblockFrame()
        cs.fill(hf, [P(p) for p in wide], [p.shape[1] * cs.isz for p in wide], [P(t) for t in cs.tabs[vertical]], vertical)
        orc.orc_deblock_frame_pass(bd, ctypes.byref(hf))
        for c in range(3):
            ph, pw = cs.planes[c].shape
            assert np.array_equal(wide[c][:ph, :pw], want[vertical][c]) and not wide[c][ph:].any() and not wide[c][:, pw:].any()


# ---------------------------------------------------------------- the device against the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("kind,bd,fmt", CLASS_CASES)
def test_classes(dev, orc, kind, bd, fmt):
    cs = case(kind, bd, fmt)
    CHECK[kind](cs, orc)
    run_gpu(dev, orc, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind", ["max", "cols1", "rows1", "cols4", "rows4", "cols16", "rows16"])
def test_range_extremes(dev, orc, kind, bd):
    """All-max and 0 / max alternating by columns, then rows (single samples as well as blocks as wide as the partitions) at the top of
    Table 43: the long filter's 65504, the weak delta's 12284 and the +-tc clips at tc' = 395."""
    run_gpu(dev, orc, case(kind, bd, "420", qp="top"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bd,fmt", [("max", 10, "444"), ("cols4", 10, "422"), ("rows4", 8, "444"), ("cols16", 10, "444"), ("rows16", 8, "422")])
def test_range_extremes_formats(dev, orc, kind, bd, fmt):
    run_gpu(dev, orc, case(kind, bd, fmt, qp="top"))


@pytest.mark.gpu
@pytest.mark.parametrize("bd,fmt", [(8, "420"), (10, "420"), (12, "420"), (10, "422"), (10, "444"), (8, "444")])
@pytest.mark.parametrize("kind", ["flat", "ramp"])
def test_four_wide_partition(dev, orc, kind, bd, fmt):
    """bs != 0 on every edge of the 4-grid in both passes: a store that rewrote a neighbour's sample shows here."""
    cs = case(kind, bd, fmt, tables="grid4")
    changed = sum(int(np.count_nonzero(a != b)) for a, b in zip(cs.oracle(orc)[0], cs.planes))
    assert changed > 500
    run_gpu(dev, orc, cs)


@pytest.mark.gpu
@pytest.mark.parametrize("tables,bd,fmt", HALF_UNIT)
def test_half_unit_at_the_border(dev, orc, tables, bd, fmt):
    """Width and height = 4 mod 8: the last 8-sample unit along an edge is half inside the picture."""
    run_gpu(dev, orc, case("flat", bd, fmt, w=132, h=68, tables=tables))


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_nothing_to_filter(dev, orc, bd):
    """Every bs 0 (whole workgroups leave), and bs != 0 with tc = 0 everywhere: the planes stay as they are."""
    for kwargs in (dict(tables="bs0"), dict(qp="zero")):
        cs = case("flat", bd, "420", w=64, h=48, ctb_log2=6, **kwargs)
        assert all(np.array_equal(a, b) for a, b in zip(cs.oracle(orc)[0], cs.planes))
        if "qp" in kwargs:
            assert cs.tabs[1][0].any() and cs.tabs[0][0].any()
        run_gpu(dev, orc, cs)

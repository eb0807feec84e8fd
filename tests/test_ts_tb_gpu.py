"""GPU parity of vvc355_ts_tb_pass, bit-exact: transform-skip blocks from 16-byte records (BDPCM on the levels, the scaling process with
ts = 1, no transform, the residual added plain, through the 64x64 unit's chroma scale, to both planes of a joint transform unit, or kept in
the arena) against the expectation tests/ts_tb_cases.py composes from the oracle, against vvc355_levels_expand + vvc355_dequant_batch where
those can express the blocks, and next to vvc355_inter_tb_pass on one picture."""
import ctypes

import numpy as np
import pytest

import inter_tb_cases as tc
import levels_cases as lc
import ts_tb_cases as ts
from ffvvc_amd import abi

pytestmark = pytest.mark.gpu

W, H = 128, 64                                               # luma size of the small pictures


def _pack(specs, every=None):
    """Packed levels with every `every`-th block forced to stay int32 (None: no packed levels at all)."""
    if every is None:
        return None
    return lc.pack_all([s["c"] for s in specs], force_int32={i for i in range(len(specs)) if i % every == every - 1})


def _block_at(specs, c, yx):
    for i, s in enumerate(specs):
        for plane in [s["c_idx"]] + ([3 - s["c_idx"]] if s["joint"] & 1 else []):
            if plane == c and s["x0"] <= yx[1] < s["x0"] + (1 << s["lw"]) and s["y0"] <= yx[0] < s["y0"] + (1 << s["lh"]):
                return (f"block {i}: {1 << s['lw']}x{1 << s['lh']} window {s['nzw']}x{s['nzh']} c_idx {s['c_idx']} joint {s['joint']} "
                        f"bdpcm {s['bdpcm']} vert {s['vert']} qp {s['qp']}")
    return "no block there"


def _check(dev, orc, pic, specs, packed_every=3, rbits=15):
    """Group, run the whole stage, compare planes (pitch padding included), arena and scale table with the expectation."""
    specs, class_first = ts.group(specs)
    offs, n = tc.arena_offsets(specs)
    pk = _pack(specs, packed_every)
    arena0 = tc.start_arena(specs, offs, n, None if pk is None else pk[1])
    want_planes, want_arena, want_table = ts.oracle_walk(orc, pic, specs, offs, arena0, rbits)
    fr = ts.Frame(pic, specs, class_first, offs, arena0, rbits, pk)
    assert fr.run(dev) == 0
    got_planes, got_arena = fr.dpic.pitched_planes(dev), fr.arena(dev)
    for c, (g, w) in enumerate(zip(got_planes, fr.dpic.expected_pitched(want_planes))):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}: {_block_at(specs, c, bad[0])}"
    bad = np.flatnonzero(got_arena != want_arena)
    assert len(bad) == 0, f"{len(bad)} arena words differ, first at {bad[0]} (block {int(np.searchsorted(offs, bad[0], side='right')) - 1})"
    if want_table is not None:
        assert np.array_equal(fr.dpic.d_table.to_host(np.int16, want_table.shape), want_table)
    return specs, class_first, offs, arena0, pk, fr, want_planes


def _layout(pw, ph, dims):
    """Shelf-pack (w, h) rectangles, tallest first, into as many pw x ph pages as it takes: (page, x, y) per rectangle; x is a multiple of
    min(w, 4)."""
    order = sorted(range(len(dims)), key=lambda i: (-dims[i][1], -dims[i][0]))
    out, page, x, y, shelf = [None] * len(dims), 0, 0, 0, 0
    for i in order:
        w, h = dims[i]
        x = (x + min(w, 4) - 1) // min(w, 4) * min(w, 4)
        if x + w > pw:
            x, y, shelf = 0, y + shelf, 0
        if y + h > ph:
            page, x, y, shelf = page + 1, 0, 0, 0
        out[i] = (page, x, y)
        x, shelf = x + w, max(shelf, h)
    return out


def _pictures(rng, bd, protos, hs=1, vs=1, lmcs=False, **kw):
    """protos: (c_idx, lw, lh, make(c_idx, x0, y0, lw, lh) -> spec).  Luma blocks are packed into W x H luma planes, chroma blocks into chroma
    planes (a position is used once over BOTH chroma planes, so that any chroma block may be a joint one), as many pictures as it takes."""
    luma = [p for p in protos if p[0] == 0]
    chroma = [p for p in protos if p[0] != 0]
    pages = {}
    for group, (pw, ph) in ((luma, (W, H)), (chroma, (W >> hs, H >> vs))):
        for p, (page, x, y) in zip(group, _layout(pw, ph, [(1 << p[1], 1 << p[2]) for p in group])):
            pages.setdefault(page, []).append(p[3](p[0], x, y, p[1], p[2]))
    out = []
    for page in sorted(pages):
        if lmcs:
            import recon_cases
            dt = np.uint8 if bd == 8 else np.uint16
            planes = [tc.unit_dc_luma(rng, bd, W, H, kw.get("size_y", 64))]
            planes += [rng.integers(0, 1 << bd, size=(H >> vs, W >> hs), dtype=np.int64).astype(dt) for _ in range(2)]
            pic = tc.Picture(planes, bd, hs, vs, model=recon_cases.ReconWork.lmcs_model(rng, bd), **kw)
        else:
            pic = tc.Picture.random(rng, bd, W, H, hs, vs, **kw)
        out.append((pic, pages[page]))
    return out


def _all_shapes():
    return [(0, lw, lh) for (lw, lh) in ts.LUMA_SHAPES] + [(1 + k % 2, lw, lh) for k, (lw, lh) in enumerate(ts.CHROMA_SHAPES)]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_every_shape_packed_and_int32_mixed(dev, orc, bd):
    """Sides 4..32 as luma and 2..32 as chroma blocks (at least 8 coefficients), random windows smaller than the block with empty tiles, every
    qp; packed and int32 blocks in the same call, plain add; then the same records with no packed levels at all."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A10 + bd)
    protos = [(c, lw, lh, lambda c, x, y, lw, lh: ts.random_spec(rng, c, x, y, lw, lh)) for (c, lw, lh) in _all_shapes()]
    protos += [(c, lw, lh, lambda c, x, y, lw, lh: ts.random_spec(rng, c, x, y, lw, lh, window=(1 << lw, 1 << lh), bits=15)) for (c, lw, lh) in _all_shapes()]
    pics = _pictures(rng, bd, protos)
    qp = 0
    for (_pic, specs) in pics:                               # every qp 0..63 at least once
        for s in specs:
            s["qp"], qp = qp % 64, qp + 1
    assert qp >= 64
    seen, small, empty = np.zeros((2, ts.NC), int), 0, 0
    for (pic, specs) in pics:
        sp, cf, *_ = _check(dev, orc, pic, specs, packed_every=3)
        seen += np.diff(np.array(cf), axis=1)
        small += sum(1 for s in sp if s["nzw"] < (1 << s["lw"]) or s["nzh"] < (1 << s["lh"]))
        empty += sum(1 for s in sp if s["nzw"] > 4 and not s["c"][:4, 4:8].any() and s["c"].any())
        _check(dev, orc, pic, specs, packed_every=None)
    assert seen.min() > 0 and small > 20 and empty > 5


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("vert", [0, 1])
def test_bdpcm_every_shape(dev, orc, vert, keep):
    """Horizontal and vertical BDPCM on every shape: small random levels, full-scale random levels (partial sums saturate here and there), the
    saturating levels of the case module (a plain prefix-sum kernel fails on them), and a window of one column (row) from which the
    accumulation fills the whole block.  KEEP: the whole slot is the residual.  Add: the picture is."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A20 + 2 * vert + keep)

    def rand(c, x, y, lw, lh):
        return ts.random_spec(rng, c, x, y, lw, lh, bdpcm=True, vert=vert, keep=keep)

    def full(c, x, y, lw, lh):
        return ts.random_spec(rng, c, x, y, lw, lh, window=(1 << lw, 1 << lh), bits=15, bdpcm=True, vert=vert, keep=keep)

    def sat(c, x, y, lw, lh):
        return ts.spec(c, x, y, lw, lh, ts.saturating_levels(1 << lw, 1 << lh, vert), 1 << lw, 1 << lh, qp=int(rng.integers(4, 40)), bdpcm=True, vert=vert, keep=keep)

    def line(c, x, y, lw, lh):
        w, h = 1 << lw, 1 << lh
        win = (w, 1) if vert else (1, h)
        lv = lc.windowed_block(rng, w, h, *win, bits=9)
        lv[0, 0] = lv[0, 0] or 7
        return ts.spec(c, x, y, lw, lh, lv, *win, qp=int(rng.integers(20, 40)), bdpcm=True, vert=vert, keep=keep)

    protos = [(c, lw, lh, make) for make in (rand, full, sat, line) for (c, lw, lh) in _all_shapes()]
    n_line = 0
    for (pic, specs) in _pictures(rng, 10, protos):
        sp, _cf, offs, arena0, _pk, fr, want_planes = _check(dev, orc, pic, specs, packed_every=4)
        for i, s in enumerate(sp):
            if s["nzw"] * s["nzh"] == (1 << s["lh"] if not vert else 1 << s["lw"]):      # the one-line windows: the residual is non-zero in every line
                res = ts.oracle_residual(orc, s, 10)
                n_line += int(res[:, -1].any() if not vert else res[-1, :].any())
        if keep:
            assert all(np.array_equal(a, b) for a, b in zip(want_planes, pic.planes))
    assert n_line >= len(_all_shapes()) // 2


@pytest.mark.parametrize("bd,rbits", [(10, 17), (12, 20)])
def test_extended_range_int32_levels(dev, orc, bd, rbits):
    """log2_transform_range above 15: int32 levels beyond 16 bits (not packable) next to small packed ones, with and without BDPCM in both
    directions; accumulations exceed 16 bits and saturate at the extended range; plain, joint and kept."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A30 + bd)
    k = [0]

    def make(c, x, y, lw, lh):
        k[0] += 1
        i = k[0]
        bits = [rbits - 1, rbits - 3, 6][i % 3]
        joint = [0, 1, 1 | 2 | 4][i % 3] if c else 0
        s = ts.random_spec(rng, c, x, y, lw, lh, window=(1 << lw, 1 << lh) if i % 2 else None, bits=bits, bdpcm=i % 4 != 0, vert=(i >> 2) & 1,
                           joint=joint, keep=i % 5 == 0)
        return s

    protos = [(c, lw, lh, make) for _ in range(2) for (c, lw, lh) in _all_shapes()]
    big = wide = 0
    for (pic, specs) in _pictures(rng, bd, protos):
        sp, _cf, _offs, _a, pk, *_ = _check(dev, orc, pic, specs, packed_every=5, rbits=rbits)
        big += sum(1 for s in sp if np.abs(s["c"]).max() > 32767)
        for s in sp:
            if s["bdpcm"]:
                acc = ts.bdpcm(orc, s["c"], s["vert"], rbits)
                wide += int(acc.max() == (1 << rbits) - 1 or acc.min() == -(1 << rbits))
    assert big > 20 and wide > 10


def _lmcs_protos(rng):
    def luma(c, x, y, lw, lh):
        return ts.random_spec(rng, c, x, y, lw, lh, bdpcm=bool(rng.integers(0, 2)), vert=bool(rng.integers(0, 2)))

    def chroma(c, x, y, lw, lh):
        return ts.random_spec(rng, c, x, y, lw, lh, bdpcm=bool(rng.integers(0, 2)), vert=bool(rng.integers(0, 2)),
                              joint=[8, 8, 8 | 1, 8 | 1 | 2 | 4, 0][int(rng.integers(0, 5))], keep=bool(rng.random() < 0.1))

    protos = [(0, lw, lh, luma) for (lw, lh) in [(2, 2), (3, 3), (4, 4), (5, 5), (3, 2), (4, 5)] for _ in range(3)]
    return protos + [(1 + k % 2, lw, lh, chroma) for k, (lw, lh) in enumerate(ts.CHROMA_SHAPES)]


@pytest.mark.parametrize("size_y", [32, 64])
@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (0, 0)])
def test_lmcs_picture_two_calls_around_the_scale_pass(dev, orc, hs, vs, size_y):
    """Chroma residual scaling at 4:2:0, 4:2:2 and 4:4:4 with units of 32 and 64: luma call, vvc355_lmcs_vpdu_scale_pass (it reads the luma the
    first call reconstructed), chroma call with joint bit 3."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A40 + 4 * hs + 2 * vs + size_y)
    scaled = luma = 0
    for (pic, specs) in _pictures(rng, 10, _lmcs_protos(rng), hs, vs, lmcs=True, size_y=size_y, ctb_log2=5 if size_y == 32 else 7):
        *_, fr, want_planes = _check(dev, orc, pic, specs, packed_every=3)
        scaled += sum(1 for s in specs if s["joint"] & 8 and not s["keep"])
        luma += int(np.any(want_planes[0] != pic.planes[0]))
        assert fr.f.size_y == size_y
    assert scaled > 10 and luma


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_large_coding_units_take_the_scale_of_their_origin(dev, orc, bd):
    """The LARGE_CUS geometry (CtbSizeY 128, 256x256 luma at 4:2:0): coding units of 128x128, 128x64 and 64x128 whose 32x32 transform-skip
    chroma blocks lie in four or two units and all take the scale of the unit of the coding unit's origin; a few of them joint, half of them
    BDPCM.  Before the device is touched the case is shown to tell that rule from the block's-own-unit rule."""
    import recon_cases
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A50 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    planes = [tc.unit_dc_luma(rng, bd, 256, 256)] + [rng.integers(0, 1 << bd, size=(128, 128), dtype=np.int64).astype(dt) for _ in range(2)]
    pic = tc.Picture(planes, bd, 1, 1, 64, 7, recon_cases.ReconWork.lmcs_model(rng, bd))
    specs = []
    for y in range(0, 256, 64):
        for x in range(0, 256, 64):
            specs.append(ts.random_spec(rng, 0, x + 8, y + 8, 4, 4, bdpcm=bool((x + y) & 64)))
    for (cx, cy, cw, chh) in tc.LARGE_CUS:
        for uy in range(cy, cy + chh, 64):
            for ux in range(cx, cx + cw, 64):
                bd_kw = dict(bdpcm=bool(rng.integers(0, 2)), vert=bool(rng.integers(0, 2)), cu=(cx, cy))
                if rng.random() < 0.25:                      # a joint transform unit: one record, both planes
                    specs.append(ts.random_spec(rng, int(rng.integers(1, 3)), ux // 2, uy // 2, 5, 5, joint=8 | 1 | (int(rng.integers(0, 4)) << 1), **bd_kw))
                else:
                    for c in (1, 2):
                        specs.append(ts.random_spec(rng, c, ux // 2, uy // 2, 5, 5, joint=8, **bd_kw))
    sp, _cf = ts.group(specs)
    offs, n = tc.arena_offsets(sp)
    by_cu, _a, table = ts.oracle_walk(orc, pic, sp, offs, tc.start_arena(sp, offs, n))
    far, differ = tc.unit_rule_split(pic, sp, table)
    assert far >= 12 and 2 * differ >= far
    _check(dev, orc, pic, specs, packed_every=3)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_joint_cbcr_one_record_two_planes(dev, orc, bd):
    """tu_joint_cbcr_residual_flag: sign x shift x coded component x scaled / unscaled, on several shapes, with and without BDPCM; both chroma
    planes are compared."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED7A60 + bd)
    shapes = [(2, 2), (3, 3), (4, 4), (5, 5), (3, 2), (2, 4), (1, 3), (3, 1), (1, 5), (4, 1)]
    protos, seen = [], set()
    k = 0
    for rep in range(2):
        for sign in (0, 2):
            for shift in (0, 4):
                for c in (1, 2):
                    for scaled in (0, 8):
                        lw, lh = shapes[k % len(shapes)]
                        joint, bdp, vert = 1 | sign | shift | scaled, bool(rep), bool(k & 1)
                        protos.append((c, lw, lh, lambda c, x, y, lw, lh, joint=joint, bdp=bdp, vert=vert:
                                       ts.random_spec(rng, c, x, y, lw, lh, joint=joint, bdpcm=bdp, vert=vert)))
                        seen.add((sign, shift, c, scaled))
                        k += 1
    assert len(seen) == 16
    protos += [(0, 4, 3, lambda c, x, y, lw, lh: ts.random_spec(rng, c, x, y, lw, lh)) for _ in range(6)]   # the scales come from reconstructed luma
    for (pic, specs) in _pictures(rng, bd, protos, lmcs=True):
        *_, want_planes = _check(dev, orc, pic, specs, packed_every=3)
        assert np.any(want_planes[1] != pic.planes[1]) and np.any(want_planes[2] != pic.planes[2])


def test_keep_leaves_the_residual_in_the_arena_and_the_picture_alone(dev, orc):
    """KEEP records, packed and int32, luma and chroma, with and without BDPCM, between records that add: the whole slot holds the residual,
    the picture under a KEEP block is untouched, and the sentinels in front of, between and behind the slots are intact."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED7A70)
    k = [0]

    def make(c, x, y, lw, lh):
        k[0] += 1
        return ts.random_spec(rng, c, x, y, lw, lh, keep=k[0] % 3 != 0, bdpcm=k[0] % 2 == 0, vert=bool(k[0] & 4))

    kept_n = 0
    for (pic, specs) in _pictures(rng, bd, [(c, lw, lh, make) for (c, lw, lh) in _all_shapes()]):
        sp, _cf, offs, arena0, pk, fr, _want = _check(dev, orc, pic, specs, packed_every=2)
        got, arena = fr.dpic.planes(dev), fr.arena(dev)
        kept = [i for i, s in enumerate(sp) if s["keep"]]
        assert any(pk[1][i]["flags"] for i in kept) and any(not pk[1][i]["flags"] for i in kept)
        kept_n += len(kept)
        mask = np.ones(arena.shape, bool)
        for i in kept:
            s = sp[i]
            w, h = 1 << s["lw"], 1 << s["lh"]
            assert np.array_equal(got[s["c_idx"]][s["y0"]:s["y0"] + h, s["x0"]:s["x0"] + w], pic.planes[s["c_idx"]][s["y0"]:s["y0"] + h, s["x0"]:s["x0"] + w])
            assert np.array_equal(arena[offs[i]:offs[i] + w * h], ts.oracle_residual(orc, s, bd).ravel())
            mask[offs[i]:offs[i] + w * h] = False
        assert np.array_equal(arena[mask], arena0[mask])
        gaps = np.ones(arena.shape, bool)
        for i, s in enumerate(sp):
            gaps[offs[i]:offs[i] + s["c"].size] = False
        assert gaps.sum() == (len(sp) + 1) * tc.GAP and np.all(arena[gaps] == tc.SENT)
    assert kept_n > 20


def _malformed_cases():
    """(name, needs a scale table, spec fields) — a spec marked bad, filed with good records of its channel type and class."""
    def chroma(lw=3, lh=3, **kw):
        return dict(c_idx=1, lw=lw, lh=lh, **kw)

    def luma(lw=3, lh=3, **kw):
        return dict(c_idx=0, lw=lw, lh=lh, **kw)

    return [
        ("a side of 64", False, luma(5, 3, rec_lw=6, cls=3)),
        ("a side of 1", False, chroma(1, 4, rec_lw=0)),
        ("fewer than 8 coefficients", False, chroma(1, 1)),
        ("an area larger than its class", False, luma(3, 3, cls=0)),
        ("a 32x32 block in class 2", False, chroma(5, 5, cls=2)),
        ("reserved flag bit 7", False, chroma(flags_or=0x80)),
        ("reserved joint bit 4", False, chroma(joint_or=0x10)),
        ("reserved joint bit 7", False, luma(joint_or=0x80)),
        ("pad byte set", False, luma(pad=1)),
        ("c_idx 3", False, chroma(flags_or=3)),
        ("c_idx 0 with joint bits", False, luma(joint=1)),
        ("luma record among the chroma records", False, luma(ch=1)),
        ("chroma record among the luma records", False, chroma(ch=0)),
        ("joint bit 3 without a scale table", False, chroma(joint=8)),
        ("coding unit's unit left of the picture", True, chroma(joint=8, flags_or=abi.TS_TU_UNIT_DX)),
        ("coding unit's unit above the picture", True, chroma(joint=8, flags_or=abi.TS_TU_UNIT_DY)),
        ("rectangle beyond the right edge", False, chroma(x_over=4)),
        ("rectangle beyond the lower edge", False, luma(y_over=4)),
        ("joint rectangle beyond the right edge", False, chroma(joint=1 | 2, x_over=8)),
        ("negative position", False, luma(x_neg=True)),
        ("coeff_off not a multiple of 4, int32 levels", False, luma(off_add=2, int32=True)),
        ("coeff_off not a multiple of 4, KEEP", False, chroma(off_add=1, keep=True)),
    ]


@pytest.mark.parametrize("case", range(22))
def test_malformed_records_are_skipped_between_good_ones(dev, orc, case):
    """Each kind of malformed record between two good ones of its class: the good ones are decoded, and planes (pitch padding included), arena
    and scale table are otherwise as before the call.  These are guards, nothing is provoked: every address the record names lies inside the
    buffers."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED7A80 + case)
    name, lmcs, kw = _malformed_cases()[case]
    if lmcs:
        import recon_cases
        planes = [tc.unit_dc_luma(rng, bd, W, H)] + [rng.integers(0, 1 << bd, size=(H // 2, W // 2), dtype=np.int64).astype(np.uint16) for _ in range(2)]
        pic = tc.Picture(planes, bd, model=recon_cases.ReconWork.lmcs_model(rng, bd))
    else:
        pic = tc.Picture.random(rng, bd, W, H)
    kw = dict(kw)
    c_idx, lw, lh = kw.pop("c_idx"), kw.pop("lw"), kw.pop("lh")
    ph, pw = pic.planes[c_idx].shape
    w, h = 1 << lw, 1 << lh
    x0, y0 = 8, 0                                            # (first unit of the picture in both axes)
    if "x_over" in kw:
        x0 = pw - w + kw.pop("x_over")
    if "y_over" in kw:
        y0 = ph - h + kw.pop("y_over")
    if kw.pop("x_neg", False):
        x0 = -4
    force_int32 = kw.pop("int32", False)
    bad = ts.random_spec(rng, c_idx, x0, y0, lw, lh, bad=True, bdpcm=bool(case & 1), vert=bool(case & 2), **kw)
    ch = kw.get("ch", int(c_idx > 0))
    cls = kw.get("cls", ts.area_class(lw, lh))
    glw, glh = [(2, 2), (3, 3), (4, 4), (4, 5)][cls]
    gc = 0 if ch == 0 else 2
    gh_ = 1 << glh
    good = [ts.random_spec(rng, gc, gx, 16, glw, glh, joint=8 if (lmcs and gc) else 0, qp=int(rng.integers(32, 46)), bdpcm=bool(k & 1))
            for k, gx in enumerate((0, 16, 32))]
    assert 16 + gh_ <= pic.planes[gc].shape[0] and ts.area_class(glw, glh) == cls
    for s in good:
        s["c"][0, 0] = 40                                    # a DC level: the residual cannot vanish
    others = [ts.random_spec(rng, 0, 96, 0, 5, 5), ts.random_spec(rng, 1, 48, 0, 3, 4), ts.random_spec(rng, 2, 48, 16, 1, 2)]
    specs = good[:2] + [bad] + good[2:] + others
    sp, class_first = ts.group(specs)
    i_bad = next(i for i, s in enumerate(sp) if s.get("bad"))
    assert not sp[i_bad - 1].get("bad") and not sp[i_bad + 1].get("bad")
    assert class_first[ch][cls] < i_bad < class_first[ch][cls + 1] - 1, name
    offs, n = tc.arena_offsets(sp)
    pk = lc.pack_all([s["c"] for s in sp], force_int32={i_bad} if force_int32 else set())
    arena0 = tc.start_arena(sp, offs, n, pk[1])
    want_planes, want_arena, want_table = ts.oracle_walk(orc, pic, sp, offs, arena0)
    dev.vvc355_clear_error()
    dev.vvc355_set_error_policy(1)
    try:
        fr = ts.Frame(pic, sp, class_first, offs, arena0, 15, pk)
        assert fr.run(dev) == 0
        got_planes, got_arena = fr.dpic.pitched_planes(dev), fr.arena(dev)
        assert dev.vvc355_last_error() == 0, ctypes.string_at(dev.vvc355_last_error_string())
    finally:
        dev.vvc355_set_error_policy(0)
    for c, (g, wnt) in enumerate(zip(got_planes, fr.dpic.expected_pitched(want_planes))):
        diff = np.argwhere(g != wnt)
        assert len(diff) == 0, f"{name}: component {c}, {len(diff)} samples differ, first at {diff[0].tolist()}"
    for s in good:                                           # the neighbours of the malformed record were decoded
        w_, h_ = 1 << s["lw"], 1 << s["lh"]
        assert np.any(got_planes[gc][s["y0"]:s["y0"] + h_, s["x0"]:s["x0"] + w_] != pic.planes[gc][s["y0"]:s["y0"] + h_, s["x0"]:s["x0"] + w_]), name
    assert np.array_equal(got_arena, want_arena), name
    if want_table is not None:
        assert np.array_equal(fr.dpic.d_table.to_host(np.int16, want_table.shape), want_table)


def test_keep_blocks_equal_levels_expand_plus_dequant_batch(dev, orc):
    """KEEP blocks without BDPCM, every shape, packed with a few int32 ones: the arena, sentinels included, is what vvc355_levels_expand +
    vvc355_dequant_batch leave on the same levels."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED7A90)
    protos = [(c, lw, lh, lambda c, x, y, lw, lh: ts.random_spec(rng, c, x, y, lw, lh, keep=True)) for (c, lw, lh) in _all_shapes()]
    for (pic, specs) in _pictures(rng, bd, protos):
        sp, _cf, offs, arena0, pk, fr, _want = _check(dev, orc, pic, specs, packed_every=5)
        old = ts.OldPath(pic, sp, offs, arena0, 15, pk)
        old.run(dev)
        a_old, a_new = old.arena(dev), fr.arena(dev)
        assert np.array_equal(a_old, a_new) and np.any(a_new != arena0)


def test_both_record_passes_on_one_picture(dev, orc):
    """vvc355_inter_tb_pass and vvc355_ts_tb_pass on disjoint blocks of one picture and one arena, in either call order: the oracle's picture;
    and channels 1 then 2 of both equals channels 3 of both."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED7AA0)
    pic = tc.Picture.random(rng, bd, W, H)
    inter, skip = [], []
    for c_idx in range(3):
        for k, cell in enumerate(ts.cells(pic, c_idx)):
            lw, lh = [(2, 2), (3, 3), (4, 4), (5, 5), (3, 4), (5, 2)][(k + c_idx) % 6] if c_idx == 0 else [(1, 3), (3, 3), (4, 4), (2, 1)][(k + c_idx) % 4]
            x, y = ts.in_cell(rng, cell, lw, lh)
            if (k + c_idx) % 2:
                inter.append(tc.random_spec(rng, c_idx, x, y, lw, lh, keep=k % 5 == 4))
            else:
                skip.append(ts.random_spec(rng, c_idx, x, y, lw, lh, bdpcm=k % 4 == 0, vert=bool(k & 2), keep=k % 5 == 2))
    inter, bin_first = tc.group(inter)
    skip, class_first = ts.group(skip)
    assert len(inter) >= 5 and len(skip) >= 5
    both = inter + skip
    offs, n = tc.arena_offsets(both)
    pk_i, pk_t = _pack(inter, 3), _pack(skip, 3)
    arena0 = tc.start_arena(both, offs, n, np.concatenate([pk_i[1], pk_t[1]]))
    want_planes, want_arena, _t = ts.oracle_walk(orc, pic, both, offs, arena0)
    f_i = tc.Frame(pic, inter, bin_first, offs[:len(inter)], arena0, 15, pk_i)
    f_t = ts.Frame(pic, skip, class_first, offs[len(inter):], arena0, 15, pk_t, shared=f_i)
    want_pitched = f_i.dpic.expected_pitched(want_planes)
    for order in ([(f_i, 3), (f_t, 3)], [(f_t, 3), (f_i, 3)], [(f_t, 1), (f_i, 1), (f_i, 2), (f_t, 2)], [(f_i, 1), (f_t, 1), (f_t, 2), (f_i, 2)]):
        f_i.reset(dev)
        for (fr, channels) in order:
            assert fr.launch(dev, channels) == 0
        got = f_i.dpic.pitched_planes(dev)
        assert all(np.array_equal(g, w) for g, w in zip(got, want_pitched)), [c for (_f, c) in order]
        assert np.array_equal(f_i.arena(dev), want_arena)
    assert any(np.any(w != p) for w, p in zip(want_planes, pic.planes))

"""GPU parity of vvc355_inter_tb_pass, bit-exact: the transform stage of the coding units outside the in-order pass from 16-byte records
(scaling process, transform types derived per block, levels from the packed stream, the residual added in the transform's epilogue: plain,
through the 64x64 unit's chroma scale, to both planes of a joint transform unit, or kept in the arena) against the oracle walk of
tests/inter_tb_cases.py, and against the path it replaces where that path can express the records."""
import ctypes

import numpy as np
import pytest

import inter_tb_cases as tc
import levels_cases as lc
from ffvvc_amd import abi

pytestmark = pytest.mark.gpu

E = abi.TU_MTS_ENABLED


def _pack(specs, every=None):
    """Packed levels with every `every`-th block forced to stay int32 (None: no packed levels at all)."""
    if every is None:
        return None
    return lc.pack_all([s["c"] for s in specs], force_int32={i for i in range(len(specs)) if i % every == every - 1})


def _check(dev, orc, pic, specs, packed_every=3, rbits=15, rule="cu"):
    """Group, run the whole stage, compare planes (pitch padding included), arena and scale table with the oracle walk."""
    specs, bin_first = tc.group(specs)
    offs, n = tc.arena_offsets(specs)
    pk = _pack(specs, packed_every)
    arena0 = tc.start_arena(specs, offs, n, None if pk is None else pk[1])
    want_planes, want_arena, want_table = tc.oracle_walk(orc, pic, specs, offs, arena0, rule, rbits)
    fr = tc.Frame(pic, specs, bin_first, offs, arena0, rbits, pk)
    assert fr.run(dev) == 0
    got_planes, got_arena = fr.dpic.pitched_planes(dev), fr.arena(dev)
    for c, (g, w) in enumerate(zip(got_planes, fr.dpic.expected_pitched(want_planes))):
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}: {_block_at(specs, c, bad[0])}"
    bad = np.flatnonzero(got_arena != want_arena)
    assert len(bad) == 0, f"{len(bad)} arena words differ, first at {bad[0]} (block {int(np.searchsorted(offs, bad[0], side='right')) - 1})"
    if want_table is not None:
        assert np.array_equal(fr.dpic.d_table.to_host(np.int16, want_table.shape), want_table)
    return specs, bin_first, offs, arena0, pk, fr, want_planes


def _block_at(specs, c, yx):
    for i, s in enumerate(specs):
        for plane in [s["c_idx"]] + ([3 - s["c_idx"]] if s["joint"] & 1 else []):
            if plane == c and s["x0"] <= yx[1] < s["x0"] + (1 << s["lw"]) and s["y0"] <= yx[0] < s["y0"] + (1 << s["lh"]):
                return f"block {i}: {1 << s['lw']}x{1 << s['lh']} c_idx {s['c_idx']} joint {s['joint']} keep {s['keep']} tu_flags {s['tu_flags']} mts {s['mts_idx']}"
    return "no block there"


def _cells(pic, c_idx):
    ph, pw = pic.planes[c_idx].shape
    return [(x, y) for y in range(0, ph, 64) for x in range(0, pw, 64)]


SHAPES = [(lw, lh) for lw in range(2, 7) for lh in range(2, 7)]
THIN = [(1, 2), (1, 3), (1, 4), (1, 5), (2, 1), (3, 1), (4, 1), (5, 1)]


def _in_cell(rng, cell, lw, lh):
    """A position inside a 64x64 cell, a multiple of 4 samples (of 2 for the narrow side of a thin block)."""
    w, h = 1 << lw, 1 << lh
    ax, ay = min(4, w), min(4, h)
    return cell[0] + int(rng.integers(0, (64 - w) // ax + 1)) * ax, cell[1] + int(rng.integers(0, (64 - h) // ay + 1)) * ay


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_every_shape_packed_and_int32_mixed(dev, orc, bd):
    """All 25 shapes as luma (three each) and chroma blocks, the thin shapes 2x4 .. 2x32 and 4x2 .. 32x2 as chroma blocks, random windows, qp,
    dep-quant; packed and int32 blocks in the same call; then the same records with no packed levels at all."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3A10 + bd)
    pic = tc.Picture.random(rng, bd, 1024, 512)
    luma, chroma = _cells(pic, 0), [(c, cell) for c in (1, 2) for cell in _cells(pic, 1)]
    rng.shuffle(luma)
    rng.shuffle(chroma)
    specs = []
    for (lw, lh) in SHAPES:
        for _ in range(3):
            specs.append(tc.random_spec(rng, 0, *_in_cell(rng, luma.pop(), lw, lh), lw, lh, max_nz=32, tu_flags=E, mts_idx=0))
        c, cell = chroma.pop()
        specs.append(tc.random_spec(rng, c, *_in_cell(rng, cell, lw, lh), lw, lh, max_nz=32))
    for (lw, lh) in THIN:
        for _ in range(2):
            c, cell = chroma.pop()
            specs.append(tc.random_spec(rng, c, *_in_cell(rng, cell, lw, lh), lw, lh))
    for k, qp in enumerate(range(52)):                       # every qp at least once
        specs[(k * 37) % len(specs)]["qp"] = qp
    sp, bf, *_ = _check(dev, orc, pic, specs, packed_every=3)
    assert all(bf[0][k + 1] > bf[0][k] for k in range(25)) and all(bf[1][k + 1] > bf[1][k] for k in range(26))
    _check(dev, orc, pic, specs, packed_every=None)


@pytest.mark.parametrize("bd,rbits", [(10, 17), (12, 20)])
def test_extended_range_takes_the_generic_arithmetic(dev, orc, bd, rbits):
    """log2_transform_range above 15: every workgroup falls back to the generic code, with levels beyond 16 bits (int32, not packable) next to
    small ones, through every epilogue: plain, scaled, joint, kept."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3A18 + bd)
    pic = tc.Picture.random(rng, bd, 512, 256, lmcs=True)
    luma, chroma = _cells(pic, 0), _cells(pic, 1)
    specs = []
    for k, cell in enumerate(luma):
        lw, lh = SHAPES[(k * 7) % 25]
        w, h = 1 << lw, 1 << lh
        nzw, nzh = min(w, 8), min(h, 8)
        c = lc.windowed_block(rng, w, h, nzw, nzh, bits=17 if k % 2 else 6)
        mts_idx = 0 if max(lw, lh) == 6 else k % 5           # no 64-point DST-7 / DCT-8
        specs.append(tc.spec(0, *_in_cell(rng, cell, lw, lh), lw, lh, c, nzw, nzh, qp=int(rng.integers(0, 40)), dep=k & 1, tu_flags=E, mts_idx=mts_idx, keep=k % 5 == 0))
    for k, cell in enumerate(chroma):
        lw, lh = (SHAPES + THIN)[(k * 5) % 33]
        joint = [0, 8, 8 | 1, 1 | 2 | 4, 8 | 1 | 2, 8 | 1 | 4][k % 6] if (1 << (lw + lh)) > 4 else 0
        specs.append(tc.random_spec(rng, 1 + k % 2, *_in_cell(rng, cell, lw, lh), lw, lh, max_nz=8, joint=joint, keep=k % 7 == 3))
    _check(dev, orc, pic, specs, packed_every=2, rbits=rbits)


@pytest.mark.parametrize("bd", [8, 10])
def test_transform_type_syntax_differs_from_block_to_block(dev, orc, bd):
    """Luma records whose tu_flags / mts_idx differ from one to the next: the four SBT flag combinations on shapes on both sides of the
    max(w, h) <= 32 rule, explicit mts_idx 0..4, MTS disabled.  One frame-wide tu_flags cannot describe this batch."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3A20 + bd)
    pic = tc.Picture.random(rng, bd, 1024, 512)
    kinds = [(E | abi.TU_SBT | hor | pos, 0) for hor in (0, abi.TU_SBT_HORIZONTAL) for pos in (0, abi.TU_SBT_POS)]
    kinds += [(E, m) for m in range(5)]                                      # explicit MTS of an inter coding unit
    kinds += [(0, 0), (abi.TU_SBT | abi.TU_SBT_HORIZONTAL, 0)]               # MTS disabled: DCT-2 whatever SBT says
    shapes = [(2, 2), (3, 3), (4, 4), (5, 5), (3, 4), (5, 3), (2, 5), (6, 5), (4, 6), (6, 6)]
    cells = _cells(pic, 0)
    rng.shuffle(cells)
    specs = []
    for (lw, lh) in shapes:
        for (tu_flags, mts_idx) in kinds:
            if max(lw, lh) == 6 and mts_idx:                                 # a 64-point DST-7 / DCT-8 does not exist: no stream codes it
                continue
            specs.append(tc.random_spec(rng, 0, *_in_cell(rng, cells.pop(), lw, lh), lw, lh, tu_flags=tu_flags, mts_idx=mts_idx))
    types = {tc.tr_type(orc, s) for s in specs}
    assert types >= {0x00, 0x11, 0x12, 0x21, 0x22}
    big_sbt = [s for s in specs if s["tu_flags"] & abi.TU_SBT and s["tu_flags"] & E and max(s["lw"], s["lh"]) == 6]
    assert big_sbt and all(tc.tr_type(orc, s) == 0 for s in big_sbt)        # beyond 32 SBT is not implicit
    assert all(tc.tr_type(orc, s) != 0 for s in specs if s["tu_flags"] & abi.TU_SBT and s["tu_flags"] & E and max(s["lw"], s["lh"]) <= 5)
    order = rng.permutation(len(specs))
    sp, bf, *_ = _check(dev, orc, pic, [specs[i] for i in order], packed_every=4)
    differ = sum(1 for a, b in zip(sp, sp[1:]) if (a["tu_flags"], a["mts_idx"]) != (b["tu_flags"], b["mts_idx"]))
    assert differ > len(sp) // 2


@pytest.mark.parametrize("hs,vs", [(1, 1), (1, 0), (0, 0)])
def test_lmcs_picture_two_calls_around_the_scale_pass(dev, orc, hs, vs):
    """A small picture with chroma residual scaling at 4:2:0, 4:2:2 and 4:4:4: luma call, vvc355_lmcs_vpdu_scale_pass, chroma call.  At
    4:2:0 the planes are also those of the old path on the same records."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED3A30 + 2 * hs + vs)
    pic = tc.Picture.random(rng, bd, 256, 128, hs, vs, lmcs=True)
    specs = tc.tiled_specs(rng, pic, [(4, 4), (3, 3), (5, 4), (2, 3)], [(3, 3), (2, 2), (4, 3), (1, 3), (5, 5), (2, 1)], scaled_frac=0.8, keep_frac=0.1,
                           tu_flags=(0, E), mts=(0, 1, 4))
    assert sum(1 for s in specs if s["joint"] & 8) > 40 and sum(1 for s in specs if s["c_idx"] and not s["joint"]) > 10
    sp, bf, offs, arena0, pk, fr, want_planes = _check(dev, orc, pic, specs, packed_every=3)
    if (hs, vs) == (1, 1):
        old = tc.OldPath(orc, pic, sp, offs, arena0, 15, pk)
        old.run(dev)
        got_old, got_new = old.dpic.planes(dev), fr.dpic.planes(dev)
        for c in range(3):
            assert np.array_equal(got_old[c], got_new[c]), f"component {c}: old and new path differ"
        keep = [i for i, s in enumerate(sp) if s["keep"]]
        a_old, a_new = old.arena(dev), fr.arena(dev)
        assert keep and all(np.array_equal(a_old[offs[i]:offs[i] + sp[i]["c"].size], a_new[offs[i]:offs[i] + sp[i]["c"].size]) for i in keep)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_joint_cbcr_one_record_two_planes(dev, orc, bd):
    """tu_joint_cbcr_residual_flag: sign x shift x coded component x scaled / unscaled on several shapes; both chroma planes are compared."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3A40 + bd)
    pic = tc.Picture.random(rng, bd, 1024, 512, lmcs=True)
    cells = _cells(pic, 1)                                                   # a joint record owns its cell in BOTH chroma planes
    shapes = [(2, 2), (3, 3), (4, 4), (5, 5), (3, 2), (2, 4), (1, 3), (3, 1)]
    specs, seen = [], set()
    k = 0
    for sign in (0, 2):
        for shift in (0, 4):
            for c in (1, 2):
                for scaled in (0, 8):
                    lw, lh = shapes[k % len(shapes)]
                    specs.append(tc.random_spec(rng, c, *_in_cell(rng, cells[k], lw, lh), lw, lh, joint=1 | sign | shift | scaled))
                    seen.add((sign, shift, c, scaled))
                    k += 1
    assert len(seen) == 16 and k <= len(cells)
    for cell in cells[k:k + 8]:                                              # and luma blocks, so that the scales come from reconstructed luma
        specs.append(tc.random_spec(rng, 0, 2 * cell[0] + 8, 2 * cell[1] + 60, 4, 3))
    *_, want_planes = _check(dev, orc, pic, specs, packed_every=3)
    assert np.any(want_planes[1] != pic.planes[1]) and np.any(want_planes[2] != pic.planes[2])


def test_keep_leaves_the_residual_in_the_arena_and_the_picture_alone(dev, orc):
    """KEEP records, packed and int32, luma and chroma, between records that add: the slot holds the oracle's residual, the picture under a
    KEEP block and every other arena word are as before the call."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED3A50)
    pic = tc.Picture.random(rng, bd, 512, 256)
    specs = []
    for k, cell in enumerate(_cells(pic, 0)):
        lw, lh = SHAPES[(k * 3) % 25]
        specs.append(tc.random_spec(rng, 0, *_in_cell(rng, cell, lw, lh), lw, lh, keep=k % 2 == 0))
    for k, cell in enumerate(_cells(pic, 1)):
        lw, lh = (SHAPES + THIN)[(k * 4) % 33]
        specs.append(tc.random_spec(rng, 1 + k % 2, *_in_cell(rng, cell, lw, lh), lw, lh, keep=k % 3 != 0))
    sp, bf, offs, arena0, pk, fr, want_planes = _check(dev, orc, pic, specs, packed_every=2)
    got, arena = fr.dpic.planes(dev), fr.arena(dev)
    kept = [i for i, s in enumerate(sp) if s["keep"]]
    assert len(kept) > 15 and any(pk[1][i]["flags"] for i in kept) and any(not pk[1][i]["flags"] for i in kept)
    mask = np.ones(arena.shape, bool)
    for i in kept:
        s = sp[i]
        w, h = 1 << s["lw"], 1 << s["lh"]
        assert np.array_equal(got[s["c_idx"]][s["y0"]:s["y0"] + h, s["x0"]:s["x0"] + w], pic.planes[s["c_idx"]][s["y0"]:s["y0"] + h, s["x0"]:s["x0"] + w])
        assert np.array_equal(arena[offs[i]:offs[i] + w * h], tc.oracle_residual(orc, s, bd).ravel())
        mask[offs[i]:offs[i] + w * h] = False
    assert np.array_equal(arena[mask], arena0[mask])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_large_coding_units_take_the_scale_of_their_origin(dev, orc, bd):
    """CtbSizeY 128, coding units of 128x128, 128x64 and 64x128 whose chroma blocks lie in four or two units: every block takes the scale
    orc_lmcs_chroma_scale_flat gives at the unit of the CODING UNIT's origin.  Before the device is touched the case is shown to tell that
    rule from the block's-own-unit rule."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED3F10 + bd)
    pic, specs = tc.large_cu_case(rng, bd)
    sp, _bf = tc.group(specs)
    offs, n = tc.arena_offsets(sp)
    by_cu, _a, table = tc.oracle_walk(orc, pic, sp, offs, tc.start_arena(sp, offs, n), "cu")
    for (cx, cy, _w, _h) in tc.LARGE_CUS:
        assert table[(cy // 64) * pic.ux + cx // 64] == tc.oracle_unit_scale(orc, pic, by_cu[0], cx // 64, cy // 64)
    far, differ = tc.unit_rule_split(pic, sp, table)
    print(f"bd {bd}: {differ} of {far} blocks outside their coding unit's first unit would take another scale by the block rule")
    assert far >= 12 and 2 * differ >= far
    _check(dev, orc, pic, specs, packed_every=3, rule="cu")


def _malformed_cases(rng):
    """(name, needs a scale table, spec maker) — every maker returns a spec marked bad that sits in the bin of shape (lw, lh) of `ch`."""
    def chroma(lw=3, lh=3, **kw):
        return dict(c_idx=1, lw=lw, lh=lh, **kw)

    def luma(lw=3, lh=3, **kw):
        return dict(c_idx=0, lw=lw, lh=lh, **kw)

    return [
        ("shape not the bin's", False, luma(4, 4, bin=tc.shape_bin(3, 3))),
        ("thin block filed under a shape bin", False, chroma(1, 3, bin=tc.shape_bin(2, 3))),
        ("shape filed under the thin bin", False, chroma(3, 3, bin=25)),
        ("a side beyond 64", False, luma(3, 3, rec_lw=7, bin=tc.shape_bin(3, 3))),
        ("reserved flag bit 6", False, luma(flags_or=0x40)),
        ("reserved flag bit 7", False, chroma(flags_or=0x80)),
        ("reserved joint_mts bit 7", False, luma(joint_mts_or=0x80)),
        ("mts_idx 5", False, luma(joint_mts_or=5 << 4)),
        ("c_idx 3", False, chroma(flags_or=3)),
        ("c_idx 0 with joint bits", False, luma(joint=1)),
        ("luma record among the chroma records", False, luma(ch=1)),
        ("joint bit 3 without a scale table", False, chroma(joint=8)),
        ("rectangle beyond the right edge", False, chroma(x_over=4)),
        ("rectangle beyond the lower edge", False, luma(y_over=4)),
        ("joint rectangle beyond the right edge", False, chroma(joint=1 | 2, x_over=8)),
        ("negative position", False, luma(x_neg=True)),
        ("coeff_off not a multiple of 4, int32 levels", False, luma(off_add=2, int32=True)),
        ("coeff_off not a multiple of 4, KEEP", False, chroma(off_add=1, keep=True)),
        ("coding unit's unit left of the picture", True, chroma(joint=8, flags_or=abi.INTER_TU_UNIT_DX)),
    ]


@pytest.mark.parametrize("case", range(19))
def test_malformed_records_are_skipped_between_good_ones(dev, orc, case):
    """Each kind of malformed record between two good ones of its bin: the good ones are decoded, and planes (pitch padding included), arena
    and scale table are otherwise as before the call.  These are guards, nothing is provoked: every address the record names lies inside the
    buffers."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED3A70 + case)
    name, lmcs, kw = _malformed_cases(rng)[case]
    pic = tc.Picture.random(rng, bd, 256, 128, lmcs=lmcs)
    kw = dict(kw)
    c_idx, lw, lh = kw.pop("c_idx"), kw.pop("lw"), kw.pop("lh")
    ph, pw = pic.planes[c_idx].shape
    w, h = 1 << lw, 1 << lh
    x0, y0 = (16 if name.startswith("coding unit's unit") else 64), 16
    if "x_over" in kw:
        x0 = pw - w + kw.pop("x_over")
    if "y_over" in kw:
        y0 = ph - h + kw.pop("y_over")
    if kw.pop("x_neg", False):
        x0 = -4
    force_int32 = kw.pop("int32", False)
    bad = tc.random_spec(rng, c_idx, x0, y0, lw, lh, bad=True, **kw)
    blw, blh = (lw, lh) if "bin" not in kw or kw["bin"] == 25 else (kw["bin"] // 5 + 2, kw["bin"] % 5 + 2)
    ch = kw.get("ch", int(c_idx > 0))
    gc = 0 if ch == 0 else 2
    if kw.get("bin") == 25:
        blw, blh = 1, 3
    good = [tc.random_spec(rng, gc, gx, 40, blw, blh, joint=8 if (lmcs and gc) else 0, qp=int(rng.integers(32, 46))) for gx in (0, 32, 96)]
    for s in good:
        s["c"][0, 0] = 40                                    # a DC level: the residual cannot vanish
    others = [tc.random_spec(rng, 0, 192, 0, 5, 5), tc.random_spec(rng, 1, 96, 0, 4, 4), tc.random_spec(rng, 2, 16, 8, 1, 2)]
    specs = good[:2] + [bad] + good[2:] + others
    sp, bin_first = tc.group(specs)
    i_bad = next(i for i, s in enumerate(sp) if s.get("bad"))
    assert not sp[i_bad - 1].get("bad") and not sp[i_bad + 1].get("bad")
    assert bin_first[ch][tc.shape_bin(blw, blh)] < i_bad < bin_first[ch][tc.shape_bin(blw, blh) + 1] - 1, name
    offs, n = tc.arena_offsets(sp)
    pk = lc.pack_all([s["c"] for s in sp], force_int32={i_bad} if force_int32 else set())
    arena0 = tc.start_arena(sp, offs, n, pk[1])
    want_planes, want_arena, want_table = tc.oracle_walk(orc, pic, sp, offs, arena0)
    dev.vvc355_clear_error()
    dev.vvc355_set_error_policy(1)
    try:
        fr = tc.Frame(pic, sp, bin_first, offs, arena0, 15, pk)
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


def test_luma_then_chroma_equals_both_at_once(dev, orc):
    """channels 1 then 2 gives what channels 3 gives on a picture without scaling; each call touches its own channel type only."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED3A80)
    pic = tc.Picture.random(rng, bd, 256, 128)
    specs = tc.tiled_specs(rng, pic, [(4, 4), (3, 3), (6, 6), (2, 2)], [(3, 3), (2, 2), (5, 5), (1, 2)], keep_frac=0.1)
    sp, bf, offs, arena0, pk, fr3, _w = _check(dev, orc, pic, specs, packed_every=3)
    both = fr3.dpic.pitched_planes(dev), fr3.arena(dev)
    fr = tc.Frame(pic, sp, bf, offs, arena0, 15, pk)
    assert fr.launch(dev, 1) == 0
    after_luma = fr.dpic.pitched_planes(dev)
    assert np.array_equal(after_luma[0], both[0][0]) and all(np.array_equal(after_luma[c], fr.dpic.host[c]) for c in (1, 2))
    assert fr.launch(dev, 2) == 0
    got = fr.dpic.pitched_planes(dev), fr.arena(dev)
    assert all(np.array_equal(a, b) for a, b in zip(got[0], both[0])) and np.array_equal(got[1], both[1])

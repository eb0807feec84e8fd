"""GPU parity of vvc355_intra_tb_pass, bit-exact: the intra transform stage from 16-byte records (scaling process, LFNST inside the transform
kernel, transform types derived per block, levels from the packed stream) against the oracle chain orc_dequant -> orc_ilfnst_transform ->
orc_derive_transform_type -> orc_itx, and against the path it replaces (levels_expand -> lfnst_batch -> itx_batch_lv per class)."""
import ctypes

import numpy as np
import pytest

import intra_tb_cases as tc
import levels_cases as lc
import recon_cases
from ffvvc_amd import abi

pytestmark = pytest.mark.gpu


def _run(dev, specs, bd, packed=None, launch_mode=0, rbits=15):
    """Group, run, and return (sorted specs, offsets, arena length, result arena, frame)."""
    specs, class_first = tc.group_by_class(specs)
    offs, n = tc.arena_offsets(specs)
    pk = None
    if packed is not None:
        pk = lc.pack_all([s["c"] for s in specs], force_int32=packed(specs))
    arena = tc.start_arena(specs, offs, n, None if pk is None else pk[1])
    fr = tc.Frame(specs, class_first, offs, arena, bd, rbits, pk, launch_mode)
    assert fr.launch(dev) == 0
    return specs, offs, n, fr.result(dev), fr


def _first_diff(got, want, specs, offs):
    bad = np.flatnonzero(got != want)
    if not len(bad):
        return ""
    k = int(np.searchsorted(offs, bad[0], side="right")) - 1
    s = specs[max(k, 0)]
    return (f"{len(bad)} arena words differ, first at {bad[0]} (block {k}: {1 << s['lw']}x{1 << s['lh']} c_idx {s['c_idx']} lfnst {s['lfnst']} "
            f"idx {s['lfnst_idx']} mode {s['mode']} tu_flags {s['tu_flags']} mts {s['mts_idx']} class {s['cls']})")


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_directed_lfnst_shapes(dev, orc, bd):
    """Every LFNST block shape x index x mode kind x dep-quant, qp over 0..51: both input sizes (8, 16), both output sizes (16, 48), both
    placements.  Packed levels and int32 levels in place, both launch shapes."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED2F10 + bd)
    shapes = [(2, 2), (3, 3), (2, 4), (4, 2), (3, 4), (4, 4), (5, 3), (5, 5), (6, 6)]
    modes = [0, 1, 18, 34, 35, 50, 66, -1, -14, 67, 73, 80]
    specs, seen = [], set()
    for (lw, lh) in shapes:
        w, h = 1 << lw, 1 << lh
        for idx in (1, 2):
            for mode in modes:
                for dep in (0, 1):
                    qp = int(rng.integers(0, 52))
                    specs.append(tc.spec(lw, lh, tc.lfnst_levels(rng, w, h, bits=int(rng.choice([3, 6, 9]))), min(w, 4), min(h, 4), 0, qp, dep,
                                         True, idx, mode, abi.TU_MTS_ENABLED | abi.TU_INTRA))
                    seen.add((tc.lfnst_nz(w, h), 48 if (w >= 8 and h >= 8) else 16, mode > 34))
    for k, qp in enumerate(range(52)):                      # every qp at least once
        specs[(k * 37) % len(specs)]["qp"] = qp
    # nz 8 with 16 outputs is the 4x4 block, nz 8 with 48 the 8x8 block, nz 16 with 16 the 4xN / Nx4 blocks, nz 16 with 48 the rest
    assert seen == {(nz, n_out, tr) for nz in (8, 16) for n_out in (16, 48) for tr in (False, True)}
    assert {m for m in modes if m < 0} and {m for m in modes if 67 <= m <= 80} and {m for m in modes if 0 <= m <= 34} and {m for m in modes if 34 < m < 67}
    want = None
    for packed, mode in ((None, 1), (None, 2), (lambda sp: {i for i in range(len(sp)) if i % 10 == 3}, 1), (lambda sp: {i for i in range(len(sp)) if i % 10 == 3}, 2)):
        sp, offs, n, got, _fr = _run(dev, specs, bd, packed, mode)
        if want is None:
            want = tc.expected_arena(orc, sp, offs, n, bd)
            assert np.any(want != tc.start_arena(sp, offs, n))
        assert np.array_equal(got, want), (packed is not None, mode, _first_diff(got, want, sp, offs))


@pytest.mark.parametrize("bd", [8, 10])
def test_transform_type_syntax_differs_from_block_to_block(dev, orc, bd):
    """Records whose tu_flags / mts_idx / lfnst_idx / c_idx differ: implicit MTS, explicit MTS 0..4, ISP (with its 1xN / 2xN / Nx1 / Nx2
    sub-partitions), MIP, ISP with LFNST (DCT-2), chroma.  One frame-wide tu_flags cannot describe this batch."""
    tc.bind_oracle(orc)
    rng = np.random.default_rng(0x5EED2F20 + bd)
    E = abi.TU_MTS_ENABLED
    specs = []

    def add(lw, lh, tu_flags, mts_idx=0, c_idx=0, lfnst=False, lfnst_idx=0, max_nz=16):
        w, h = 1 << lw, 1 << lh
        qp, dep = int(rng.integers(0, 52)), int(rng.integers(0, 2))
        if lfnst:
            specs.append(tc.spec(lw, lh, tc.lfnst_levels(rng, w, h), min(w, 4), min(h, 4), c_idx, qp, dep, True, lfnst_idx, int(rng.integers(-14, 81)),
                                 tu_flags, mts_idx))
        else:
            nzw, nzh = int(rng.integers(1, min(w, max_nz) + 1)), int(rng.integers(1, min(h, max_nz) + 1))
            specs.append(tc.spec(lw, lh, lc.windowed_block(rng, w, h, nzw, nzh), nzw, nzh, c_idx, qp, dep, False, lfnst_idx, 0, tu_flags, mts_idx))

    square_ish = [(2, 2), (3, 2), (2, 3), (3, 3), (4, 3), (4, 4), (5, 4), (4, 5), (5, 5), (2, 5), (5, 2)]
    for (lw, lh) in square_ish + [(6, 6), (6, 4), (3, 6)]:
        add(lw, lh, E | abi.TU_INTRA)                                                # implicit MTS: DST-7 for sizes 4..16
        add(lw, lh, abi.TU_INTRA)                                                    # MTS off: DCT-2
        add(lw, lh, E | abi.TU_INTRA | abi.TU_MIP)                                   # MIP: not implicit
        add(lw, lh, E | abi.TU_INTRA, c_idx=1 + (lw & 1))                            # chroma: DCT-2
    for (lw, lh) in square_ish:
        for mts_idx in range(5):                                                     # explicit MTS: DCT-2 / DST-7 / DCT-8 pairs
            add(lw, lh, E | abi.TU_EXPLICIT_MTS_INTRA | abi.TU_INTRA, mts_idx)
        add(lw, lh, E | abi.TU_EXPLICIT_MTS_INTRA | abi.TU_INTRA, 0, lfnst=True, lfnst_idx=1 + (lh & 1))
    # ISP sub-partitions: 1xN / 2xN / Nx1 / Nx2 and the 4-wide / 4-high ones
    for (lw, lh) in [(0, 4), (0, 5), (0, 6), (1, 3), (1, 4), (1, 5), (1, 6), (4, 0), (5, 0), (6, 0), (3, 1), (4, 1), (5, 1), (6, 1), (2, 3), (2, 4), (3, 2), (4, 2),
                     (3, 3), (4, 3), (5, 3)]:
        for _ in range(3):
            add(lw, lh, E | abi.TU_INTRA | abi.TU_ISP)
        add(lw, lh, abi.TU_INTRA | abi.TU_ISP)                                       # ISP is implicit only with MTS enabled
    for (lw, lh) in [(2, 2), (2, 3), (2, 4), (3, 2), (4, 2), (3, 3), (4, 3), (5, 3), (3, 4)]:
        for idx in (1, 2):                                                           # ISP with LFNST: DCT-2, LFNST on the sub-partition
            add(lw, lh, E | abi.TU_INTRA | abi.TU_ISP, lfnst=True, lfnst_idx=idx)
            add(lw, lh, E | abi.TU_INTRA | abi.TU_ISP, lfnst=False, lfnst_idx=idx)   # ... and a block of such a unit without the LFNST bit
    for (lw, lh) in [(2, 2), (3, 3), (4, 4), (3, 4)]:
        add(lw, lh, E | abi.TU_INTRA, c_idx=1, lfnst=True, lfnst_idx=2)              # chroma LFNST (dual tree)
    kinds = {(s["tu_flags"], s["mts_idx"], bool(s["lfnst_idx"]), s["c_idx"] > 0) for s in specs}
    assert len({k[0] for k in kinds}) >= 6 and {k[1] for k in kinds} == set(range(5))
    types = {orc.orc_derive_transform_type(s["tu_flags"], s["mts_idx"], s["lfnst_idx"], s["c_idx"], 1 << s["lw"], 1 << s["lh"]) for s in specs}
    assert types >= {0x00, 0x11, 0x12, 0x21, 0x22, 0x01, 0x10}
    order = rng.permutation(len(specs))
    specs = [specs[i] for i in order]
    want = None
    for packed, mode in ((None, 1), (lambda sp: {i for i in range(len(sp)) if i % 7 == 2}, 2), (lambda sp: set(), 1), (None, 2)):
        sp, offs, n, got, _fr = _run(dev, specs, bd, packed, mode)
        if want is None:
            want = tc.expected_arena(orc, sp, offs, n, bd)
        assert np.array_equal(got, want), (packed is not None, mode, _first_diff(got, want, sp, offs))


@pytest.mark.parametrize("keep_classes", [(0, 1, 2, 3, 4), (1, 3), (4,), (0,)])
def test_picture_population_packed_and_in_place(dev, orc, keep_classes):
    """The intra transform blocks of a recon_cases picture, LFNST on a fifth of the luma blocks as the bench draws them; int32 levels in
    place and packed, both launch shapes, against the oracle and against today's path.  Subsets leave classes (and the 64x64 class) empty."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED2F30)
    work = recon_cases.ReconWork(rng, 768, 512, 7, 1, 1, split=(0.6, 0.1))
    specs = [s for s in tc.picture_specs(rng, work.tbs) if s["cls"] in keep_classes]
    if keep_classes == (0, 1, 2, 3, 4):
        assert {s["cls"] for s in specs} == {0, 1, 2, 3, 4}
        assert sum(s["lfnst"] for s in specs) > 50
        assert any(s["lw"] < 2 for s in specs)              # ISP's narrow sub-partitions are part of the population
    specs, class_first = tc.group_by_class(specs)
    offs, n = tc.arena_offsets(specs)
    want = tc.expected_arena(orc, specs, offs, n, bd)

    force = {i for i in range(len(specs)) if i % 10 == 7}
    levels, lv = lc.pack_all([s["c"] for s in specs], force_int32=force)
    packed_frac = float((lv["flags"] == 0).mean())
    print(f"classes {keep_classes}: {len(specs)} blocks, class_first {class_first}, {packed_frac:.3f} packed")
    assert packed_frac >= 0.85

    results = {}
    for name, pk in (("in place", None), ("packed", (levels, lv))):
        arena = tc.start_arena(specs, offs, n, None if pk is None else lv)
        if pk is not None:
            i = next(k for k in range(len(specs)) if not lv[k]["flags"])
            assert np.all(arena[offs[i] - tc.GAP:offs[i] + specs[i]["c"].size] == tc.SENT)      # a packed block's slot holds no levels
        for mode in (1, 2):
            fr = tc.Frame(specs, class_first, offs, arena, bd, 15, pk, mode)
            assert fr.launch(dev) == 0
            got = fr.result(dev)
            assert np.array_equal(got, want), (name, mode, _first_diff(got, want, specs, offs))
            results[(name, mode)] = got
    assert np.array_equal(results[("packed", 1)], results[("packed", 2)])
    fr = tc.Frame(specs, class_first, offs, tc.start_arena(specs, offs, n, lv), bd, 15, (levels, lv), 0)      # the library's choice
    assert fr.launch(dev) == 0 and np.array_equal(fr.result(dev), want)

    old = tc.OldPath(specs, class_first, offs, tc.start_arena(specs, offs, n, lv), bd, 15, (levels, lv))
    old.launch(dev)
    got_old = old.result(dev)
    assert np.array_equal(got_old, results[("packed", 2)]), _first_diff(results[("packed", 2)], got_old, specs, offs)


def test_contract_violations_are_skipped_not_executed(dev, orc):
    """A block filed under too small a class, the LFNST bit on a 2x8 block, reserved flag bits, an LFNST index of 3: the kernel writes
    nothing for them (their slots keep the start arena), every other block is right, and no HIP error is recorded.  The inputs lie well
    inside device memory; this checks the guard, nothing is provoked."""
    tc.bind_oracle(orc)
    bd = 10
    rng = np.random.default_rng(0x5EED2F40)

    def good():
        out = []
        for (lw, lh) in [(2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (1, 3), (3, 4), (2, 4)] * 6:
            w, h = 1 << lw, 1 << lh
            if lw >= 2 and lh >= 2 and rng.random() < 0.4:
                out.append(tc.spec(lw, lh, tc.lfnst_levels(rng, w, h), min(w, 4), min(h, 4), 0, int(rng.integers(0, 52)), int(rng.integers(0, 2)), True,
                                   int(rng.integers(1, 3)), int(rng.integers(-14, 81))))
            else:
                nzw, nzh = int(rng.integers(1, min(w, 16) + 1)), int(rng.integers(1, min(h, 16) + 1))
                out.append(tc.spec(lw, lh, lc.windowed_block(rng, w, h, nzw, nzh), nzw, nzh, 0, int(rng.integers(0, 52)), int(rng.integers(0, 2))))
        return out

    def bad_class(cls):
        s = tc.spec(4, 4, lc.windowed_block(rng, 16, 16, 8, 8), 8, 8, cls=cls)
        s["bad"] = True
        return s

    def bad_lfnst_2x8():
        s = tc.spec(1, 3, lc.windowed_block(rng, 2, 8, 2, 4), 2, 4, lfnst=True, lfnst_idx=1, mode=20)
        s["bad"] = True
        return s

    def bad_reserved():
        s = tc.spec(3, 3, lc.windowed_block(rng, 8, 8, 4, 4), 4, 4)
        s["bad"], s["extra_flags"] = True, 0x40
        return s

    def bad_lfnst_idx():
        s = tc.spec(3, 3, tc.lfnst_levels(rng, 8, 8), 4, 4, lfnst=True, lfnst_idx=3, mode=20)
        s["bad"] = True
        return s

    dev.vvc355_clear_error()
    dev.vvc355_set_error_policy(1)
    try:
        for bads in ([bad_class(0), bad_class(1), bad_class(1)], [bad_lfnst_2x8(), bad_lfnst_2x8()], [bad_reserved(), bad_lfnst_idx()]):
            specs = good()
            for k, b in enumerate(bads):
                specs.insert(5 + 11 * k, b)
            for packed in (None, lambda sp: {i for i in range(len(sp)) if i % 9 == 1}):
                for mode in (1, 2):
                    sp, offs, n, got, fr = _run(dev, specs, bd, packed, mode)
                    skipped = {i for i, s in enumerate(sp) if s.get("bad")}
                    assert len(skipped) == len(bads)
                    want = fr.arena0.copy()
                    for i, s in enumerate(sp):
                        if i not in skipped:
                            want[offs[i]:offs[i] + s["c"].size] = tc.oracle_block(orc, s, bd).ravel()
                    assert np.array_equal(got, want), (packed is not None, mode, _first_diff(got, want, sp, offs))
                    for i in skipped:
                        if fr.lv is not None and not fr.lv[i]["flags"]:        # a packed block's slot: the sentinel stays
                            assert np.all(got[offs[i]:offs[i] + sp[i]["c"].size] == tc.SENT)
                    assert dev.vvc355_last_error() == 0, ctypes.string_at(dev.vvc355_last_error_string())
    finally:
        dev.vvc355_set_error_policy(0)

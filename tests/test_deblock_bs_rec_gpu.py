"""GPU: vvc355_deblock_bs_rec_pass — boundary strengths, luma maximum filter lengths and the chroma transform sizes straight from the unit
records, one workgroup per CTU with a one-unit halo — bit-exact against the oracle's restatement of vvc_deblock_bs (vvc_filter.c:308-783) on
the generator's own unit-by-unit tables, against the table path on the device (vvc355_tab_fill_pass + vvc355_deblock_bs_pass), with records
in any order inside a CTU, luma only, without tb_*_c, and with holes and malformed records (the completeness rule of include/vvc_mi355.h)."""
import ctypes

import numpy as np
import pytest

import bs_rec_cases as rc
from ffvvc_amd import batch

pytestmark = pytest.mark.gpu


def _assert_equal(got, want, names):
    lines = rc.mismatches(got, want, names)
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("i", range(len(rc.CASES)))
def test_outputs_equal_the_oracle(dev, orc, i):
    t, want = rc.case(orc, i)
    got = rc.run_device(dev, t, rc.grouped(t))                 # every output pre-filled with 0xEE: the device writes every entry itself
    _assert_equal(got, rc.expected(t, want), t.OUT + rc.TB_C)


def test_outputs_equal_the_table_path_on_the_device(dev, orc):
    """1480x840, CTU 128: vvc355_tab_fill_pass with all three record kinds, then vvc355_deblock_bs_pass, from the same records."""
    t, _ = rc.case(orc, len(rc.CASES))
    groups = rc.grouped(t)
    d_rec = [batch.DeviceBuffer.from_host(g[0].view(np.uint8)) for g in groups]
    d_first = [batch.DeviceBuffer.from_host(g[1]) for g in groups]
    tabs = {}
    for name in t.IN + t.OUT:
        a = getattr(t, name)
        keep = name in ("ref_poc", "slice_idx", "col_bd", "row_bd")            # everything else is written on the device
        tabs[name] = batch.DeviceBuffer.from_host(a if keep else np.full(a.nbytes, 0xEE, np.uint8))
    fill = t.fill_frame(d_rec[0].ptr, d_rec[1].ptr, d_rec[2].ptr, tuple(len(g[0]) for g in groups), lambda n: tabs[n].ptr, tuple(d.ptr for d in d_first))
    d_fill = batch.DeviceBuffer.from_host(np.frombuffer(bytes(fill), np.uint8))
    dev.vvc355_tab_fill_pass(None, d_fill.ptr, ctypes.addressof(fill))
    f = t.frame(lambda n: tabs[n].ptr)
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    dev.vvc355_deblock_bs_pass(None, d_f.ptr, ctypes.addressof(f))
    dev.vvc355_stream_sync(None)
    want = {name: tabs[name].to_host(np.uint8, (t.th, t.tw)) for name in t.OUT + rc.TB_C}
    assert set(np.unique(want["bs10"])) == {0, 1, 2}, "the table path left nothing to compare"
    got = rc.run_device(dev, t, groups)
    _assert_equal(got, want, t.OUT + rc.TB_C)


def test_record_order_inside_a_ctu_does_not_matter(dev, orc):
    t, want = rc.case(orc, 2)
    rng = np.random.default_rng(rc.SEED + 100)
    shuffled = [r[rng.permutation(len(r))] for r in t.records()]           # group_per_ctu sorts by CTU only (stable): the shuffle survives inside
    groups = rc.grouped(t, shuffled)
    assert not np.array_equal(groups[0][0], rc.grouped(t)[0][0]) and not np.array_equal(groups[1][0], rc.grouped(t)[1][0])
    _assert_equal(rc.run_device(dev, t, groups), rc.expected(t, want), t.OUT + rc.TB_C)


def test_luma_only(dev, orc):
    """n_comp = 1 without tree-1 records: the luma outputs as ever, the chroma outputs and tb_*_c untouched."""
    t, want = rc.case(orc, 2)
    cu, tu, mv = t.records()
    groups = rc.grouped(t, (cu, tu[(tu["flags"] & 0x80) == 0], mv))
    got = rc.run_device(dev, t, groups, n_comp=1)
    luma = tuple(n for n in t.OUT if n not in rc.OUT_C)
    assert len(luma) == 6
    _assert_equal(got, want, luma)
    for name in rc.OUT_C + rc.TB_C:
        assert np.all(got[name] == 0xEE), f"{name} was written"


def test_tb_size_tables_are_optional(dev, orc):
    t, want = rc.case(orc, 2)
    got = rc.run_device(dev, t, rc.grouped(t), tb_c=False)
    _assert_equal(got, want, t.OUT)
    for name in rc.TB_C:
        assert np.all(got[name] == 0xEE), f"{name} was written"


def _pick(t, recs, sel, where):
    """Index of the smallest record among recs[sel] that lies in the interior of its CTU ("interior"), ends on its CTU's right edge with a
    CTU to the right ("right"), or on its bottom edge with a CTU below ("bottom")."""
    ctb = 1 << t.ctb_log2
    x0, y0, w, h = (recs[k].astype(np.int64) for k in ("x0", "y0", "w", "h"))
    lx, ly = x0 & (ctb - 1), y0 & (ctb - 1)
    inner = (lx > 0) & (ly > 0) & (lx + w < ctb) & (ly + h < ctb) & (x0 + w < t.width) & (y0 + h < t.height)
    cond = {"interior": inner, "right": (lx + w == ctb) & (x0 + w < t.width), "bottom": (ly + h == ctb) & (y0 + h < t.height)}[where]
    idx = np.nonzero(sel & cond)[0]
    assert len(idx), where
    return int(idx[np.argmin((w * h)[idx])])


def test_holes_and_malformed_records(dev, orc):
    """Case 2 with six records removed (a coding unit, a tree-0 and a tree-1 transform unit, each once in the interior of a CTU and once on a
    CTU's right or bottom edge, where the hole is seen through the next CTU's halo) and three malformed records added, which must paint
    nothing: the full picture's oracle output with zeros exactly where the completeness rule says."""
    t, want = rc.case(orc, 2)
    cu, tu, mv = t.records()
    tree1 = (tu["flags"] & 0x80) != 0
    all_cu = np.ones(len(cu), bool)
    drop_cu = {_pick(t, cu, all_cu, "interior"), _pick(t, cu, all_cu, "right")}
    drop_tu = {_pick(t, tu, ~tree1, "interior"), _pick(t, tu, ~tree1, "bottom"), _pick(t, tu, tree1, "interior"), _pick(t, tu, tree1, "right")}
    assert len(drop_cu) == 2 and len(drop_tu) == 4
    cu = np.delete(cu, sorted(drop_cu))
    tu = np.delete(tu, sorted(drop_tu))
    ctb = 1 << t.ctb_log2
    bad_cu = np.array([(ctb + ctb - 8, ctb + 16, 16, 8, 3, 0)], cu.dtype)                     # sticks out of CTU (1, 1) to the right
    bad_tu = np.array([(2 * ctb + 8, 8, 0, 16, 0x11, 0), (ctb + 16, 2 * ctb + 8, 6, 8, 0x9e, 0)], tu.dtype)        # zero width (tree 0); w = 6 (tree 1)
    cu, tu = np.concatenate([cu, bad_cu]), np.concatenate([tu, bad_tu])                     # appended: last in their CTU, they would paint last
    assert not rc.well_formed(t, cu)[-1] and not rc.well_formed(t, tu)[-2:].any()
    exp, zeroed = rc.expected_with_holes(t, want, cu, tu)
    n_zeroed = int((zeroed[0] | zeroed[1]).sum())
    assert 0 < n_zeroed < 0.05 * t.tw * t.th, n_zeroed                                          # zeroing everything does not pass
    assert any(np.any(want[name][zeroed[int(name[2]) if name.startswith("bs") else int(name[1])]] != 0) for name in t.OUT), "no zeroed entry was non-zero"
    got = rc.run_device(dev, t, rc.grouped(t, (cu, tu, mv)))
    _assert_equal(got, exp, t.OUT + rc.TB_C)

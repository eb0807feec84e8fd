"""GPU: vvc355_col_mvf_pass against the numpy expectation of col_mvf_cases (tests/test_col_mvf_cpu.py pins it to the header's packing and to
H.266 clause 8.5.2.15).  Every comparison is exact and covers every byte of the `col` allocation: the entries, the col_stride padding and the
slack in front of and behind the array.

1. directed tables of noise, n_jobs = 0, COMPRESS on and off; 2. the whole range of a vector component; 3. the DMVR pictures: the full
dmvr_mvf table against the overlay of jobs and records on the unrefined table, both against the packing of the oracle's tab_dmvr_mvf, which
tests/golden/ref_inter.json pins to the reference; 4. directed overlay jobs; 5. graph capture; 6. a refused frame; 7. vvc355_download_async
into pinned memory and vvc355_col_mvf_scatter."""
import ctypes

import numpy as np
import pytest

import affine_gpm_cases as agc
import col_mvf_cases as cm
import inter_frame_cases as ifc
import ref_inter_cases as ic
from ffvvc_amd import abi

pytestmark = pytest.mark.gpu
C = abi.COL_MVF_COMPRESS


# ---------------------------------------------------------------------------------------------------------------- 1. directed tables

@pytest.mark.parametrize("case", cm.DIRECTED, ids=[f"{c[0]}x{c[1]}" for c in cm.DIRECTED])
def test_directed_tables(dev, case):
    width, height, mvf_stride, col_stride = case
    gw, gh = cm.grid(width, height)
    assert (mvf_stride == 0 or mvf_stride > width // 4) and (col_stride == 0 or col_stride > gw)
    seen = set()
    for shift in range(4):                          # every entry, the only one of 4x4 included, with each pred_flag
        table = cm.directed_table(1, width, height, mvf_stride, shift)
        d_table = cm.up(table)
        used = table[:, :width // 4]
        seen |= {int(v) for v in used[0::2, 0::2]["pred_flag"].reshape(-1)}
        for flags in (0, C):
            run = cm.ColRun(dev, width, height, d_table.ptr, mvf_stride, col_stride, flags)
            want = cm.pack(used, bool(flags))
            assert want.shape == (gh, gw, 2, 2)
            bad = run.run(want)
            assert not bad, f"shift {shift}: {bad}"
        assert np.array_equal(d_table.to_host(np.uint8, (table.nbytes,)), table.view(np.uint8).reshape(-1)), "the pass wrote to the table"
    assert seen == {0, 1, 2, 3}
    # the noise the entry must not show is there: a table with the other fields, the unused lists and the odd positions zeroed packs to the same
    clean = np.zeros_like(used)
    e, ce = used[0::2, 0::2], clean[0::2, 0::2]
    ce["pred_flag"] = e["pred_flag"]
    for l in range(2):
        on = ((e["pred_flag"] >> l) & 1).astype(bool)
        ce["mv"][:, :, l] = np.where(on[..., None], e["mv"][:, :, l], 0)
        ce["ref_idx"][:, :, l] = np.where(on, e["ref_idx"][:, :, l], 0)
    assert not np.array_equal(clean.view(np.uint8), np.ascontiguousarray(used).view(np.uint8)) and np.array_equal(cm.pack(clean, True), cm.pack(used, True))


# ---------------------------------------------------------------------------------------------------------------- 2. the whole range

def test_whole_range_of_a_component(dev):
    table = cm.whole_range_table()
    mv = table[0::2, 0::2]["mv"]
    assert np.array_equal(np.sort(mv.reshape(-1)), np.arange(-(1 << 17), 1 << 17))
    d_table = cm.up(table)
    for flags in (C, 0):
        run = cm.ColRun(dev, 2048, 2048, d_table.ptr, flags=flags)
        bad = run.run(cm.pack(table, bool(flags)))
        assert not bad, bad
        got_mv, got_ref, got_pf = cm.unpack(run.entries())
        assert np.array_equal(got_mv, cm.compress(mv) if flags else mv) and (got_pf == 3).all() and np.array_equal(got_ref, table[0::2, 0::2]["ref_idx"])
    assert int(cm.compress(mv).max()) == 1 << 17               # the value that needs the nineteenth bit went through


# ---------------------------------------------------------------------------------------------------------------- 3. the DMVR pictures

@pytest.mark.parametrize("name", cm.DMVR_PICTURES)
def test_dmvr_pictures(dev, orc, name):
    pic, want = cm.dmvr_picture(name), cm.oracle_run(orc, name)
    if name in cm.LISTED_DMVR:
        assert ic.sha(ic.mvf_bytes(want.dmvr)) == ic.load_golden()[name]["dmvr"], f"{name}: the oracle's tab_dmvr_mvf is not the reference's"
    assert cm.refined_points(pic, want)[0], "no refined grid point: the two ways could not differ from the unrefined table"
    full, lean = cm.InterRun(dev, pic, True), cm.InterRun(dev, pic, False)
    full.issue()
    lean.issue()
    runs = [(flags, full.hand_back(dev, flags), lean.hand_back(dev, flags, col_stride=cm.grid(pic.width, pic.height)[0] + 5)) for flags in (0, C)]
    for flags, a, b in runs:
        assert a.frame.n_jobs == 0 and a.frame.mvf == full.d_dmvr.ptr and b.frame.n_jobs == pic.n_jobs > 0 and b.frame.mvf == lean.d_mvf.ptr
        assert a.issue() == 0 and b.issue() == 0                    # behind the inter stage on the same stream, no synchronisation in between
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    dmvr = full.d_dmvr.to_host(np.uint8, (pic.mvf.nbytes,)).view(ifc.MVF_DT).reshape(pic.mvf.shape)
    assert not ic.dmvr_differences(pic, want.dmvr, dmvr, label="oracle"), "the device's full tab_dmvr_mvf is not the oracle's"
    for flags, a, b in runs:
        expect = cm.pack(want.dmvr, bool(flags))
        assert not np.array_equal(expect, cm.pack(pic.mvf, bool(flags))), "the refinement does not show in the entries"
        for how, run in (("the full table", a), ("the overlay of jobs and records", b)):
            bad = run.mismatch(expect)
            assert not bad, f"{name}, {how}: {bad}"
        assert np.array_equal(a.entries(), b.entries())
    # the unrefined table was only read
    assert np.array_equal(lean.d_mvf.to_host(np.uint8, (pic.mvf.nbytes,)), pic.mvf.view(np.uint8).reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- 4. directed overlay jobs

def overlay_case(seed=0):
    """A 48x32 picture of noise and twelve jobs: the two off-grid shapes, an aligned 16x16, one without DMVR, and eight that set_dmvr_info
    could not have made (a position that is no multiple of 4, a side of 12, 4 or 32, a rectangle that leaves the picture), each next to
    entries that must stay."""
    width, height = 48, 32
    table = cm.directed_table(20 + seed, width, height, shift=1)
    rects = [(4, 0, 8, 16, 1), (16, 12, 16, 8, 1), (32, 16, 16, 16, 1), (0, 16, 16, 16, 0),
             (18, 16, 8, 8, 1), (16, 18, 8, 8, 1), (0, 0, 12, 8, 1), (24, 0, 8, 4, 1), (40, 24, 16, 8, 1), (32, 24, 8, 16, 1), (-4, 8, 8, 8, 1), (16, 0, 32, 8, 1)]
    rng = np.random.default_rng([cm.SEED, 4, seed])
    jobs = np.zeros(len(rects), agc.BIPRED_JOB_DT)
    jobs["mv"] = rng.integers(-4000, 4000, size=(len(rects), 4))                 # the unrefined motion: not what the overlay stores
    jobs["bdof"], jobs["pred_flag"] = 1, 3
    for j, (x, y, w, h, d) in zip(jobs, rects):
        j["x"], j["y"], j["w"], j["h"], j["dmvr"] = x, y, w, h, d
    recs = rng.integers(-(1 << 17), 1 << 17, size=(len(rects), 8)).astype(np.int32)
    assert [cm.job_ok(*r[:4], width, height) for r in rects] == [True] * 4 + [False] * 8
    return width, height, table, rects, jobs, recs


def test_directed_overlay_jobs(dev):
    width, height, table, rects, jobs, recs = overlay_case()
    d_table, d_jobs, d_recs = cm.up(table), cm.up(jobs), cm.up(recs)
    for flags in (0, C):
        plain = cm.pack(table, bool(flags))
        want = cm.overlay(plain, rects, recs, width, height, bool(flags))
        changed = {(int(gx), int(gy)) for gy, gx in np.argwhere((want != plain).any(axis=(2, 3)))}
        # 8x16 at x = 4: one column, two rows; 16x8 at y = 12: two columns, one row; the aligned 16x16: four, of which two are intra and stay zero
        covered = {(1, 0), (1, 1), (2, 2), (3, 2), (4, 2), (5, 2), (4, 3), (5, 3)}
        assert changed == {(gx, gy) for gx, gy in covered if plain[gy, gx, 0, 1] >> cm.MV_BITS} and len(changed) == 6
        run = cm.ColRun(dev, width, height, d_table.ptr, 0, 9, flags, d_jobs.ptr, d_recs.ptr, len(rects))
        bad = run.run(want)
        assert not bad, bad
        got = run.entries()
        assert np.array_equal(got & cm.KEEP_MASK, plain & cm.KEEP_MASK), "the overlay changed flags or ref_idx"
    assert np.array_equal(d_jobs.to_host(np.uint8, (jobs.nbytes,)), jobs.view(np.uint8).reshape(-1))
    assert np.array_equal(d_recs.to_host(np.int32, recs.shape), recs)


# ---------------------------------------------------------------------------------------------------------------- 5. graph capture

def test_pass_captured_in_a_graph(dev):
    width, height, table, rects, jobs, recs = overlay_case()
    _, _, other, _, _, other_recs = overlay_case(1)
    d_table, d_jobs, d_recs = cm.up(table), cm.up(jobs), cm.up(recs)
    run = cm.ColRun(dev, width, height, d_table.ptr, 0, 0, C, d_jobs.ptr, d_recs.ptr, len(rects))
    expect = lambda t, r: cm.overlay(cm.pack(t, True), rects, r, width, height, True)      # noqa: E731
    s = dev.vvc355_stream_create()
    try:
        dev.vvc355_graph_begin(s)
        ret = run.issue(s)
        g = dev.vvc355_graph_end(s)
        assert ret == 0 and g
        dev.vvc355_stream_sync(s)
        assert np.array_equal(run.download(), run.image), "recorded, not run"
        for rep, (t, r) in enumerate(((table, recs), (other, other_recs), (table, recs))):
            dev.vvc355_upload(d_table.ptr, t.ctypes.data, t.nbytes)
            dev.vvc355_upload(d_recs.ptr, r.ctypes.data, r.nbytes)
            run.reset()
            dev.vvc355_graph_launch(g, s)
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
            bad = run.mismatch(expect(t, r))
            assert not bad, f"replay {rep}: {bad}"
        assert run.mismatch(expect(other, other_recs))
        dev.vvc355_graph_destroy(g)
    finally:
        dev.vvc355_stream_destroy(s)


# ---------------------------------------------------------------------------------------------------------------- 6. a refused frame

def test_refused_frame_leaves_col_untouched(dev):
    width, height = 136, 72
    table = cm.directed_table(30, width, height)
    d_table = cm.up(table)
    run = cm.ColRun(dev, width, height, d_table.ptr, flags=C)
    for field, value, code in (("width", 138, abi.COL_MVF_E_SIZE), ("height", 0, abi.COL_MVF_E_SIZE), ("mvf_stride", 33, abi.COL_MVF_E_STRIDE),
                               ("col_stride", 16, abi.COL_MVF_E_STRIDE), ("mvf", 0, abi.COL_MVF_E_TABLES), ("col", run.frame.col + 8, abi.COL_MVF_E_TABLES),
                               ("n_jobs", 3, abi.COL_MVF_E_JOBS), ("n_jobs", -1, abi.COL_MVF_E_JOBS), ("flags", 2, abi.COL_MVF_E_FLAGS),
                               ("col", d_table.ptr + 48, abi.COL_MVF_E_OVERLAP)):
        keep = getattr(run.frame, field)
        setattr(run.frame, field, value)
        assert run.issue() == code, field
        setattr(run.frame, field, keep)
    assert dev.vvc355_col_mvf_pass(None, None, ctypes.addressof(run.frame)) == abi.COL_MVF_E_FRAME
    assert dev.vvc355_col_mvf_pass(None, run.d_frame.ptr, None) == abi.COL_MVF_E_FRAME
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    assert np.array_equal(run.download(), run.image), "a refused frame wrote to col"
    bad = run.run(cm.pack(table, True))
    assert not bad, f"the same frame once it is valid: {bad}"


# ---------------------------------------------------------------------------------------------------------------- 7. the host leg

def test_download_async_and_scatter_give_the_oracles_table(dev, orc):
    name = "R0"
    pic, want = cm.dmvr_picture(name), cm.oracle_run(orc, name)
    gw, gh = cm.grid(pic.width, pic.height)
    lean = cm.InterRun(dev, pic, False)
    run = lean.hand_back(dev, 0)
    nbytes = gw * gh * cm.ENTRY
    host = dev.vvc355_host_alloc(nbytes)
    assert host and run.col_stride == gw
    try:
        ctypes.memset(host, 0xEE, nbytes)
        s = dev.vvc355_stream_create()
        try:
            lean.issue(s)
            assert run.issue(s) == 0
            dev.vvc355_download_async(s, host, run.frame.col, nbytes)          # behind the pass, no synchronisation in between
            dev.vvc355_stream_sync(s)                                           # the parser's wait for the collocated picture
            assert dev.vvc355_last_error() == 0
        finally:
            dev.vvc355_stream_destroy(s)
        tab = pic.mvf.copy()                                                    # tab_dmvr_mvf as the parser leaves it
        dev.vvc355_col_mvf_scatter(host, gw, pic.width, pic.height, tab.ctypes.data, pic.width // 4)
    finally:
        dev.vvc355_host_free(host)
    got, ref = tab[0::2, 0::2], want.dmvr[0::2, 0::2]
    assert np.array_equal(got["pred_flag"], ref["pred_flag"])
    for l in range(2):
        on = ((ref["pred_flag"] >> l) & 1).astype(bool)
        assert on.any() and np.array_equal(got["mv"][:, :, l][on], ref["mv"][:, :, l][on]) and not got["mv"][:, :, l][~on].any()
        assert np.array_equal(got["ref_idx"][:, :, l][on], ref["ref_idx"][:, :, l][on]) and (got["ref_idx"][:, :, l][~on] == -1).all()
    assert not np.array_equal(got["mv"], pic.mvf[0::2, 0::2]["mv"]), "the refinement did not arrive"
    # nothing else of the host table changed: the other fields, and the positions nobody reads
    for f in ("hpel_if_idx", "bcw_idx", "ciip_flag", "pad_"):
        assert np.array_equal(tab[f], pic.mvf[f])
    mask = np.ones(tab.shape, bool)
    mask[0::2, 0::2] = False
    assert np.array_equal(tab[mask], pic.mvf[mask])
    # and a parser that compresses what it reads gets what the COMPRESS entries would have given it
    assert np.array_equal(cm.compress(got["mv"]), cm.unpack(cm.pack(tab, True))[0])

"""GPU: vvc355_mvf_unit_pass — the MvField table written on the device from one 64-byte record per prediction unit — against the numpy
restatement of the three storage rules (mvf_unit_cases.expect_table / expect_affine_cus, which tests/test_mvf_unit_cpu.py holds to a scalar
loop over vvc_mvs.c:282-491 and to hand-worked values).  EVERY byte of the table allocation is compared (0xEE where nothing may be
written: uncovered entries, the pitch padding, a row below the picture) and every byte of the vvc355_affine_cu allocation (0xDD).

PLAIN pictures, the affine sweep (25 shapes x both models x pred_flag 1 / 2 / 3 x four control-point regimes), the GPM sweep (14 shapes x 64
partitions x four list combinations), a mixed picture against vvc355_tab_fill_pass on the expanded vvc355_mv_rec list and through
vvc355_deblock_bs_rec_pass both ways, affine pictures whose field comes from control points through vvc355_affine_frame_pass against the
oracle's affine block functions, malformed and misfiled records between good ones, link NONE, graph capture, a refused frame.

The 128x128 PLAIN unit lies in a 136x136 picture: it does not fit the 136x72 ones."""
import ctypes

import numpy as np
import pytest

import affine_gpm_cases as agc
import bs_cases
import bs_rec_cases as rc
import mvf_unit_cases as mc
import ref_inter_cases as ic
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu


def _hold(dev, g, units, first, pitch=None, n_cus=0, prof_disabled=0, cus=None):
    """Run the pass on a sentinel table (and sentinel affine records) and compare every byte with the numpy side; returns (table, cus)."""
    table = mc.sentinel_table(g, pitch)
    cus = mc.sentinel_cus(n_cus) if cus is None else cus
    want, want_cus = table.copy(), cus.copy()
    mc.expect_table(g, units, first, want, len(cus))
    mc.expect_affine_cus(g, units, first, want_cus, prof_disabled)
    got, got_cus, ret = mc.run_device(dev, g, units, first, table, cus, prof_disabled)
    assert ret == 0, f"vvc355_mvf_unit_pass refused the frame: {ret}"
    assert dev.vvc355_last_error() == 0
    bad = mc.table_mismatch(got, want)
    assert not bad, bad
    if len(cus):
        bad = mc.cus_mismatch(got_cus, want_cus)
        assert not bad, bad
    return got, got_cus


@pytest.mark.parametrize("ctb_log2,size", [(5, (136, 72)), (6, (136, 72)), (7, (136, 72)), (7, (136, 136))])
def test_plain_pictures(dev, ctb_log2, size):
    g, units, first = mc.plain_picture(ctb_log2, *size)
    got, _ = _hold(dev, g, units, first, pitch=g.tw + (ctb_log2 - 4))              # a pitch wider than the picture
    covered = np.any(got.view(np.uint8).reshape(got.shape + (24,)) != 0xEE, axis=-1)
    assert covered[:g.th, :g.tw].all() and not covered[g.th:].any() and not covered[:, g.tw:].any()


def test_more_than_1024_records_in_a_ctu(dev):
    """Two 128x128 CTUs of 4x4 units, 1024 records each, with malformed records in front: the second chunk of a CTU's records."""
    g, units, first = mc.plain_picture(7, 256, 128, modes=(1,))
    assert len(units) == 2048
    junk = np.array([mc.plain(128, 0, 4, 4, mc.mvfield(pred_flag=3)) for _ in range(40)], mc.UNIT_DT)          # filed under CTU 0: not inside it
    units = np.concatenate([junk, units])
    first = np.array([0, first[1] + 40, first[2] + 40], np.int32)
    assert int(np.count_nonzero(mc.placed(g, units, first, 0))) == 2048
    _hold(dev, g, units, first)


@pytest.mark.parametrize("shape", mc.AFFINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_affine_sweep(dev, shape):
    for k, (g, units, first) in enumerate(mc.affine_pictures(shape)):
        _hold(dev, g, units, first, pitch=g.tw + k % 3, n_cus=len(units), prof_disabled=int(k % 4 == 3))
    g, units, first = mc.affine_pictures(shape)[0]
    _hold(dev, g, units, first, n_cus=len(units), prof_disabled=1)


@pytest.mark.parametrize("shape", mc.GPM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpm_sweep(dev, shape):
    for k, (g, units, first) in enumerate(mc.gpm_pictures(shape)):
        _hold(dev, g, units, first, pitch=g.tw + k % 2)


@pytest.fixture(scope="module")
def mixed():
    t = bs_cases.BsTables(np.random.default_rng(mc.SEED + 3), 200, 136, ctb_log2=6)
    return (t,) + mc.mixed_picture([c[:4] for c in t.cu_recs])


def _tab_fill(dev, t, g, recs, rfirst, table):
    """vvc355_tab_fill_pass with the motion records alone on a copy of `table`."""
    d_tab = batch.DeviceBuffer.from_host(table.view(np.uint8))
    d_mv, d_first = batch.DeviceBuffer.from_host(recs.view(np.uint8)), batch.DeviceBuffer.from_host(rfirst)
    f = t.fill_frame(0, 0, d_mv.ptr, (0, 0, len(recs)), lambda name: d_tab.ptr if name == "mvf" else 0, (0, 0, d_first.ptr))
    f.mvf_pitch = table.shape[1]
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    dev.vvc355_tab_fill_pass(None, d_f.ptr, ctypes.addressof(f))
    dev.vvc355_stream_sync(None)
    return d_tab


def test_mixed_picture_equals_tab_fill_on_the_expanded_records(dev, mixed):
    t, g, units, first, n_aff = mixed
    got, _ = _hold(dev, g, units, first, n_cus=n_aff)
    for merge in (True, False):
        recs, rfirst = mc.expand(g, units, first, n_aff, merge)
        table = mc.sentinel_table(g)
        d_tab = _tab_fill(dev, t, g, recs, rfirst, table)
        other = d_tab.to_host(np.uint8, (table.nbytes,)).view(mc.MVF_DT).reshape(table.shape)
        bad = mc.table_mismatch(got[:g.th, :g.tw], other[:g.th, :g.tw])
        assert not bad, bad


def test_boundary_strengths_are_equal_both_ways(dev, mixed):
    """vvc355_deblock_bs_rec_pass on the table this pass wrote and on the table vvc355_tab_fill_pass wrote from the expanded records."""
    t, g, units, first, n_aff = mixed
    (cu, cu_first), (tu, tu_first), _ = rc.grouped(t)
    up = lambda a: batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a)          # noqa: E731
    d_cu, d_cu_first, d_tu, d_tu_first = up(cu), up(cu_first), up(tu), up(tu_first)
    side = {n: up(getattr(t, n)) for n in ("ref_poc", "slice_idx", "col_bd", "row_bd")}
    results = []
    for way in ("units", "mv_recs"):
        table = np.zeros((g.th, g.tw), mc.MVF_DT)
        if way == "units":
            run = mc.DeviceRun(dev, g, units, first, table, mc.sentinel_cus(n_aff))
            assert run.issue() == 0
            d_tab = run.d_tab
        else:
            d_tab = _tab_fill(dev, t, g, *mc.expand(g, units, first, n_aff), table)
        sentinel = np.full((t.th, t.tw), 0xEE, np.uint8)
        bufs = {name: up(sentinel) for name in t.OUT + rc.TB_C}
        bufs.update(side, mvf=d_tab)
        f = rc.rec_frame(t, (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr), lambda name: bufs[name].ptr)
        d_f = up(np.frombuffer(bytes(f), np.uint8))
        assert dev.vvc355_deblock_bs_rec_pass(None, d_f.ptr, ctypes.addressof(f)) == 0
        dev.vvc355_stream_sync(None)
        results.append({name: bufs[name].to_host(np.uint8, (t.th, t.tw)) for name in t.OUT})
    lines = rc.mismatches(results[0], results[1], t.OUT)
    assert not lines, "\n".join(lines)
    assert all(np.any(results[0][n] != 0xEE) for n in t.OUT) and np.any(results[0]["bs10"] == 1)          # written, and the motion rule decided somewhere


@pytest.mark.parametrize("bd", [8, 10])
def test_affine_picture_from_control_points(dev, orc, bd):
    """An affine picture whose motion field, PROF switches and offsets come from control points: this pass, then vvc355_affine_frame_pass, on
    one stream; the planes against the oracle's affine block functions run on the numpy table and diff_mv."""
    rng = np.random.default_rng(mc.SEED + 70 + bd)
    pic = ic.Picture(f"mvf-unit-{bd}", rng, bd, 1, 6, (200, 136), "A")
    g = mc.Geo(pic.width, pic.height, pic.ctb_log2)
    units = []
    for i, cu in enumerate(pic.aff):
        x, y, w, h = (int(cu[k]) for k in ("x0", "y0", "cb_width", "cb_height"))
        m = pic.mvf[y // 4, x // 4]
        model = int(rng.integers(1, 3))
        cp = mc.rand_cp(rng, mc.REGIMES[int(rng.integers(0, 3))], w, h, model)
        units.append(mc.affine(x, y, w, h, model, int(m["pred_flag"]), cp, m["ref_idx"], 0, int(m["bcw_idx"]), link=i))
    units, first = mc.group(g, units)
    assert len(units) >= 10
    clean_mvf, clean_aff = pic.mvf.copy(), pic.aff.copy()
    pic.mvf.view(np.uint8)[:] = 0xEE                                                                     # only affine units are read: the rest stays unwritten
    table = pic.mvf.view(mc.MVF_DT)
    mc.expect_table(g, units, first, table, len(units))
    pic.aff["prof_flags"], pic.aff["diff_mv"] = 0xDD, 0x5D5D
    start_aff = pic.aff.copy()
    mc.expect_affine_cus(g, units, first, pic.aff.view(mc.CU_DT))
    assert pic.aff["prof_flags"].any() and pic.aff["prof_flags"].max() <= 3 and not np.array_equal(pic.aff["diff_mv"], clean_aff["diff_mv"])
    want = ic.run_picture(orc, "orc", pic, stages="A").planes

    up = lambda a: batch.DeviceBuffer.from_host(np.ascontiguousarray(a).view(np.uint8) if a.dtype.kind == "V" else np.ascontiguousarray(a))          # noqa: E731
    dt = ic.px(bd)
    pitches = [batch.plane_pitch(d[0], pic.isz) for d in pic.dims]
    pitched = [batch.to_pitched(np.full((ph, pw), pic.sentinel, dt)) for (pw, ph) in pic.dims]
    d_dst = [up(p) for p in pitched]
    d_ref = [[[up(batch.to_pitched(pic.refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
    reft = agc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], [[pitches] * 2] * 2)
    d_reft, d_sl, d_lut = up(np.frombuffer(bytes(reft), np.uint8)), up(np.frombuffer(bytes(pic.slices), np.uint8)), up(pic.lut)
    sentinel = np.zeros(pic.mvf.shape, mc.MVF_DT)
    sentinel.view(np.uint8)[:] = 0xEE
    run = mc.DeviceRun(dev, g, units, first, sentinel, start_aff.view(mc.CU_DT))
    d_jl, d_jc = batch.DeviceBuffer(pic.n_aff_jobs * agc.AFFINE_JOB_DT.itemsize), batch.DeviceBuffer(max(64, pic.n_aff_chroma_jobs() * agc.BIPRED_JOB_DT.itemsize))
    f = pic.frame([b.ptr for b in d_dst], pitches, run.d_tab.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr)
    frame = abi.AffineFrame(pic=f, cus=run.d_cus.ptr, jobs_luma=d_jl.ptr, jobs_chroma=d_jc.ptr, n_cus=len(pic.aff), n_jobs=pic.n_aff_jobs)
    d_frame = up(np.frombuffer(bytes(frame), np.uint8))
    assert run.issue() == 0
    dev.vvc355_affine_frame_pass(None, bd, d_frame.ptr, ctypes.addressof(frame))
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    got_tab, got_cus = run.download()
    assert not mc.table_mismatch(got_tab, table) and not mc.cus_mismatch(got_cus, pic.aff.view(mc.CU_DT))
    planes = [b.to_host(p.dtype, p.shape)[:, :d[0]] for b, p, d in zip(d_dst, pitched, pic.dims)]
    lines = ic.plane_differences(pic, want, planes, label="oracle")
    assert not lines, "\n".join(lines)
    assert sum(int(np.count_nonzero(p != pic.sentinel)) for p in planes) > 10000
    pic.mvf[:], pic.aff[:] = clean_mvf, clean_aff


def test_malformed_and_misfiled_records_between_good_ones(dev):
    """A 200x136 picture at CTU 64 tiled with good records of all kinds; malformed records of every kind listed in the header, a good
    rectangle filed under the wrong CTU, records in no CTU's range and a ctu_first that decreases: the good ones exact, nothing else touched."""
    t = bs_cases.BsTables(np.random.default_rng(mc.SEED + 5), 200, 136, ctb_log2=6)
    g, units, first, n_aff = mc.mixed_picture([c[:4] for c in t.cu_recs], seed=1)
    m1, m2, m0, cp = mc.mvfield(pred_flag=1, mv=((1, 2), (3, 4))), mc.mvfield(pred_flag=2), mc.mvfield(pred_flag=0), np.full((2, 3, 2), 77)
    bad = [mc.plain(64, 64, 0, 8, m1), mc.plain(64, 64, 8, 6, m1), mc.plain(66, 64, 8, 8, m1), mc.plain(120, 64, 16, 8, m1), mc.plain(64, 120, 8, 16, m1),
           mc.plain(0, 0, 8, 8, m1), mc.plain(128, 64, 8, 8, m1), mc.plain(192, 64, 16, 8, m1), mc.plain(-4, 64, 8, 8, m1),
           mc._unit(64, 64, 8, 8, 3, body=m1.tobytes()), mc._unit(64, 64, 8, 8, 200, body=m1.tobytes()),
           mc.affine(64, 64, 4, 8, 1, 1, cp, link=0), mc.affine(64, 64, 8, 24, 1, 1, cp, link=0), mc.affine(64, 64, 8, 8, 0, 1, cp, link=0),
           mc.affine(64, 64, 8, 8, 3, 1, cp, link=0), mc.affine(64, 64, 8, 8, 1, 0, cp, link=0), mc.affine(64, 64, 8, 8, 1, 1, cp, link=n_aff),
           mc.affine(64, 64, 8, 8, 1, 1, cp, link=0xFFFFFFFE),
           mc.gpm(64, 64, 4, 8, 3, m1, m2), mc.gpm(64, 64, 64, 8, 3, m1, m2), mc.gpm(64, 64, 8, 64, 3, m1, m2), mc.gpm(64, 64, 8, 8, 64, m1, m2),
           mc.gpm(64, 64, 8, 8, 3, m0, m2), mc.gpm(64, 64, 8, 8, 3, m1, mc.mvfield(pred_flag=3))]
    bad = np.array(bad, mc.UNIT_DT)
    padded = np.array([mc.plain(64, 64, 8, 8, m1), mc.affine(64, 64, 8, 8, 1, 1, cp, link=0), mc.gpm(64, 64, 8, 8, 3, m1, m2)], mc.UNIT_DT)
    padded["pad_"] = (1, 2, 255)
    bad = np.concatenate([bad, padded])
    rs = 5                                                         # CTU (1, 1): the malformed records go first, in the middle and last in its range
    r0, r1 = int(first[rs]), int(first[rs + 1])
    assert r1 - r0 >= 2
    mid = (r0 + r1) // 2
    third = len(bad) // 3
    q = np.concatenate([units[:r0], bad[:third], units[r0:mid], bad[third:2 * third], units[mid:r1], bad[2 * third:], units[r1:]])
    qfirst = first.copy()
    qfirst[rs + 1:] += len(bad)
    ok = mc.placed(g, q, qfirst, n_aff)
    assert int(np.count_nonzero(~ok)) == len(bad) and int(np.count_nonzero(ok)) == len(units)
    rules = {mc.rule(g, r, rs, n_aff) for r in bad}
    assert rules == set(range(1, 14)), rules
    want_ref = mc.sentinel_table(g, g.tw + 3)
    mc.expect_table(g, units, first, want_ref, n_aff)
    got, got_cus = _hold(dev, g, q, qfirst, pitch=g.tw + 3, n_cus=n_aff)
    assert not mc.table_mismatch(got, want_ref)                    # the picture without the malformed records
    # a ctu_first that decreases: CTU 1's range swallows CTU 2's records (not inside CTU 1: skipped) and CTU 2's own range is empty; and a last
    # range that reaches past n_units: the records there are never read
    tail = np.concatenate([units, np.array([mc.plain(192, 128, 8, 8, m2)] * 3, mc.UNIT_DT)])
    dfirst = first.copy()
    assert first[3] > first[2]
    dfirst[2], dfirst[-1] = first[3] + 1, len(tail)
    ok = mc.placed(g, tail[:len(units)], dfirst, n_aff)
    assert not ok[first[2]:first[3]].any() and ok[:first[2]].all() and ok[first[3]:].all()
    run = mc.DeviceRun(dev, g, tail, dfirst, mc.sentinel_table(g), mc.sentinel_cus(n_aff), n_cus=n_aff)
    run.f.n_units = len(units)                                     # the three at the end lie past n_units
    run.d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(run.f), np.uint8))
    assert run.issue() == 0
    dev.vvc355_stream_sync(None)
    want, want_cus = mc.sentinel_table(g), mc.sentinel_cus(n_aff)
    mc.expect_table(g, tail[:len(units)], dfirst, want, n_aff)
    mc.expect_affine_cus(g, tail[:len(units)], dfirst, want_cus)
    got, got_cus = run.download()
    assert not mc.table_mismatch(got, want) and not mc.cus_mismatch(got_cus, want_cus)
    uncovered = np.all(want.view(np.uint8).reshape(want.shape + (24,)) == 0xEE, axis=-1)[:g.th, :g.tw]
    assert 0.02 < uncovered.mean() < 0.5                           # CTU 2 (and what CTU 3 lost) stayed as it was


def test_link_none(dev):
    """AFFINE records without a link: the table as ever, and no vvc355_affine_cu is written — with an array to write to, and with none."""
    g, units, first = mc.affine_pictures((16, 16))[0]
    units = units.copy()
    linked = units["link"].copy()
    units["link"][::2] = mc.NONE
    got, got_cus = _hold(dev, g, units, first, n_cus=len(units))
    raw = got_cus.view(np.uint8).reshape(len(units), -1)
    idx = linked[::2].astype(int)
    assert np.all(raw[idx] == 0xDD) and not np.all(raw[linked[1::2].astype(int), 16:] == 0xDD)
    units["link"] = mc.NONE
    _hold(dev, g, units, first, n_cus=0)


def test_pass_captured_in_a_graph(dev):
    g, units, first = mc.affine_pictures((8, 8))[0]
    n = len(units)
    other = units.copy()
    other["body"], other["aux"], other["pf"], other["ref_idx"] = (units[k][::-1] for k in ("body", "aux", "pf", "ref_idx"))          # other units' motion in the same places
    table, cus = mc.sentinel_table(g, g.tw + 1), mc.sentinel_cus(n)
    run = mc.DeviceRun(dev, g, units, first, table, cus)

    def expect(u):
        want, want_cus = table.copy(), cus.copy()
        mc.expect_table(g, u, first, want, n)
        mc.expect_affine_cus(g, u, first, want_cus)
        return want, want_cus
    s = dev.vvc355_stream_create()
    try:
        dev.vvc355_graph_begin(s)
        ret = run.issue(s)
        graph = dev.vvc355_graph_end(s)
        assert ret == 0 and graph
        dev.vvc355_stream_sync(s)
        got, got_cus = run.download()
        assert not mc.table_mismatch(got, table) and not mc.cus_mismatch(got_cus, cus), "recorded, not run"
        for rep, u in enumerate((units, other, units)):
            dev.vvc355_upload(run.d_units.ptr, u.ctypes.data, u.nbytes)
            dev.vvc355_upload(run.d_tab.ptr, table.ctypes.data, table.nbytes)
            dev.vvc355_upload(run.d_cus.ptr, cus.ctypes.data, cus.nbytes)
            dev.vvc355_graph_launch(graph, s)
            dev.vvc355_stream_sync(s)
            assert dev.vvc355_last_error() == 0
            got, got_cus = run.download()
            want, want_cus = expect(u)
            bad = mc.table_mismatch(got, want) or mc.cus_mismatch(got_cus, want_cus)
            assert not bad, f"replay {rep}: {bad}"
        assert mc.table_mismatch(*[expect(u)[0] for u in (units, other)])
        dev.vvc355_graph_destroy(graph)
    finally:
        dev.vvc355_stream_destroy(s)


def test_refused_frame_leaves_the_table_alone(dev):
    g, units, first = mc.plain_picture(6)
    table = mc.sentinel_table(g)
    for kw, code in ((dict(mvf_pitch=g.tw - 1), abi.MVF_UNIT_E_PITCH), (dict(ctb_log2=4), abi.MVF_UNIT_E_CTB), (dict(ctb_width=g.cw + 1), abi.MVF_UNIT_E_GRID),
                     (dict(n_affine_cus=2), abi.MVF_UNIT_E_AFFINE)):
        run = mc.DeviceRun(dev, g, units, first, table)
        for k, v in kw.items():
            setattr(run.f, k, v)
        run.d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(run.f), np.uint8))
        assert run.issue() == code, kw
        dev.vvc355_stream_sync(None)
        got, _ = run.download()
        assert np.all(got.view(np.uint8) == 0xEE), kw
    assert dev.vvc355_last_error() == 0

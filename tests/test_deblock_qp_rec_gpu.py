"""GPU: vvc355_deblock_qp_rec_pass — fc->tab.qp[LUMA] / [CB] / [CR] painted on the device from the unit records and their QP sidecars, one
workgroup per CTU — equal to the table setters' definition restated in numpy (qp_rec_cases.expected) on the bs_rec_cases pictures and on
directed single-CTU pictures, with records in any order inside a CTU, with holes and malformed records, luma only, and end to end:
MvField fill, vvc355_deblock_bs_rec_pass, this pass and both vvc355_deblock_frame_pass directions against the oracle's deblocking on the
oracle's bS tables and the painter's QP tables.  Outputs are pre-filled with 0xEE and have a pitch above the picture's width in units,
so that an entry the device did not write, or pitch padding it did write, shows."""
import ctypes

import numpy as np
import pytest

import bs_rec_cases as rc
import qp_rec_cases as qc
from ffvvc_amd import batch

pytestmark = pytest.mark.gpu


def _assert_equal(got, want, g, names=qc.TABLES):
    lines = qc.mismatches(got, want, g, names)
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("i", range(len(rc.CASES)))
def test_tables_equal_the_painter(dev, orc, i):
    p = qc.picture(orc, i)
    pitch = qc.odd_pitch(p.g) if i % 2 else qc.aligned_pitch(p.g)           # dword stores on aligned rows, byte stores on the others
    _assert_equal(qc.run_device(dev, p, pitch), qc.expected(p), p.g)


@pytest.mark.parametrize("name", qc.DIRECTED)
def test_directed_single_ctu_pictures(dev, name):
    p = qc.directed(name)
    _assert_equal(qc.run_device(dev, p), qc.expected(p), p.g)


def test_record_order_inside_a_ctu_does_not_matter(dev, orc):
    p = qc.picture(orc, 2)
    rng = np.random.default_rng(qc.SEED + 100)
    ctus = qc.split(p)
    for c in ctus:
        for k in (0, 2):                                  # records and their sidecar move together
            perm = rng.permutation(len(c[k]))
            c[k], c[k + 1] = c[k][perm], c[k + 1][perm]
    q = qc.join(p.g, ctus)
    assert not np.array_equal(q.cu, p.cu) and not np.array_equal(q.tu, p.tu)
    assert np.array_equal(q.cu_first, p.cu_first) and np.array_equal(q.tu_first, p.tu_first)
    want = qc.expected(p)
    assert all(np.array_equal(qc.expected(q)[n], want[n]) for n in qc.TABLES)
    _assert_equal(qc.run_device(dev, q, qc.odd_pitch(p.g)), want, p.g)


def _smallest(recs, sel):
    idx = np.nonzero(sel)[0]
    assert len(idx)
    return int(idx[np.argmin((recs["w"].astype(int) * recs["h"].astype(int))[idx])])


def test_holes_and_malformed_records(dev, orc):
    """Case 2 (6 x 4 CTUs of 64) with two CTUs emptied (one of every record, one of its transform units only), single records removed, and
    malformed records added whose sidecar bytes are not 0: zero size, misaligned, sticking out of the CTU, and a well-formed rectangle
    filed under the neighbouring CTU.  Zeros where nothing well-formed covers, everything else unchanged."""
    p = qc.picture(orc, 2)
    g, full = p.g, qc.expected(p)
    ctb = 1 << g.ctb_log2
    ctus = qc.split(p)
    ctus[3] = [a[:0] for a in ctus[3]]
    ctus[g.cw + 2][2], ctus[g.cw + 2][3] = ctus[g.cw + 2][2][:0], ctus[g.cw + 2][3][:0]
    for rs in (0, 2 * g.cw + 1):                         # the smallest coding unit and the smallest tree-1 transform unit of two more CTUs
        c = ctus[rs]
        k = _smallest(c[0], np.ones(len(c[0]), bool))
        c[0], c[1] = np.delete(c[0], k), np.delete(c[1], k)
        k = _smallest(c[2], (c[2]["flags"] & 0x80) != 0)
        c[2], c[3] = np.delete(c[2], k), np.delete(c[3], k, axis=0)
    rs, ox, oy = g.cw + 1, ctb, ctb                       # CTU (1, 1): the malformed records go FIRST and LAST in its lists
    bad = [(ox + 8, oy + 8, 0, 16), (ox + 8, oy + 8, 16, 0), (ox + 6, oy + 16, 8, 8), (ox + 16, oy + 16, 6, 8), (ox + ctb - 8, oy + 16, 16, 8),
           (ox + 16, oy + ctb - 4, 8, 8), (ox - 4, oy + 8, 8, 8), (ox + ctb + 8, oy + 8, 16, 16), (ox + 8, oy - ctb + 8, 16, 16)]
    bad_cu = np.array([b + (0, 0) for b in bad], qc.REC_DT)
    bad_tu = np.array([b + (0x86, 0) for b in bad], qc.REC_DT)
    c = ctus[rs]
    half = len(bad) // 2
    c[0], c[1] = np.concatenate([bad_cu[:half], c[0], bad_cu[half:]]), np.concatenate([np.full(half, 0x55, np.int8), c[1], np.full(len(bad) - half, 0x55, np.int8)])
    c[2] = np.concatenate([bad_tu[:half], c[2], bad_tu[half:]])
    c[3] = np.concatenate([np.full((half, 2), 0x55, np.int8), c[3], np.full((len(bad) - half, 2), 0x55, np.int8)])
    q = qc.join(g, ctus)
    n_bad = int(np.count_nonzero(~qc.paints(g, q.cu, q.cu_first)))
    assert n_bad == len(bad) and int(np.count_nonzero(~qc.paints(g, q.tu, q.tu_first))) == len(bad)
    want = qc.expected(q)
    for n in qc.TABLES:
        holes = (want[n] == 0) & (full[n] != 0)
        assert 0 < int(holes.sum()) < 0.15 * g.tw * g.th, (n, int(holes.sum()))            # zeroing everything does not pass
        assert np.array_equal(want[n][~holes], full[n][~holes]) and not np.any(want[n] == 0x55), n
    per = ctb // 4
    assert np.array_equal(want["qp_y"][per:2 * per, 2 * per:3 * per], full["qp_y"][per:2 * per, 2 * per:3 * per])          # CTU (2, 1) keeps qp_y
    assert not want["qp_c0"][per:2 * per, 2 * per:3 * per].any()                                                           # and lost its qp_c
    _assert_equal(qc.run_device(dev, q, qc.odd_pitch(g)), want, g)


def test_luma_only(dev, orc):
    """n_comp = 1 with tu = ctu_first_tu = tu_qp_c = qp_c = 0: qp_y as ever."""
    p = qc.picture(orc, 1)
    got = qc.run_device(dev, p, n_comp=1, with_tu=False)
    _assert_equal(got, qc.expected(p), p.g, ("qp_y",))
    # and with everything passed: qp_c is not written
    got = qc.run_device(dev, p, n_comp=1)
    _assert_equal(got, qc.expected(p), p.g, ("qp_y",))
    for n in ("qp_c0", "qp_c1"):
        assert np.all(got[n].view(np.uint8) == 0xEE), f"{n} was written"


def test_tree0_records_alone_leave_qp_c_zero(dev, orc):
    """Case 2 with its tree-1 transform units removed, n_comp = 3: tu_qp_c of tree-0 records is never looked at."""
    p = qc.picture(orc, 2)
    ctus = qc.split(p)
    for c in ctus:
        keep = (c[2]["flags"] & 0x80) == 0
        c[2], c[3] = c[2][keep], c[3][keep]
    q = qc.join(p.g, ctus)
    assert len(q.tu) > 0 and np.count_nonzero(q.tu_qp_c) > len(q.tu)
    want = qc.expected(q)
    assert not want["qp_c0"].any() and not want["qp_c1"].any() and want["qp_y"].any()
    _assert_equal(qc.run_device(dev, q), want, p.g)


@pytest.mark.parametrize("i", qc.E2E)
def test_deblocking_end_to_end_from_records(dev, orc, i):
    t, _ = rc.case(orc, i)
    p = qc.picture(orc, i)
    planes, dims, dbp = qc.e2e_inputs(orc, i)
    want = qc.e2e_oracle(orc, i, qc.expected(p))
    changed = sum(int(np.count_nonzero(a != b)) for a, b in zip(planes, want))
    assert changed > 2000, changed

    keep = []
    up = lambda a: keep.append(batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a)) or keep[-1]          # noqa: E731
    (cu, cu_first), (tu, tu_first), (mv, mv_first) = rc.grouped(t)
    assert np.array_equal(cu, p.cu) and np.array_equal(tu, p.tu)
    sentinel = np.full((t.th, t.tw), 0xEE, np.uint8)
    tabs = {name: up(sentinel) for name in t.OUT + rc.TB_C + qc.TABLES}
    tabs["mvf"] = batch.DeviceBuffer(t.mvf.nbytes)
    for name in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
        tabs[name] = up(getattr(t, name))
    d_cu, d_cu_first, d_tu, d_tu_first, d_cu_qp, d_tu_qp_c = (up(a) for a in (cu, cu_first, tu, tu_first, p.cu_qp, p.tu_qp_c))
    # the MvField table, the boundary strengths and the QP tables: three launches on one stream, nothing comes back in between
    rc.fill_mvf(dev, t, mv, mv_first, tabs["mvf"], None, keep)
    bf = rc.rec_frame(t, (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr), lambda name: tabs[name].ptr)
    assert dev.vvc355_deblock_bs_rec_pass(None, up(np.frombuffer(bytes(bf), np.uint8)).ptr, ctypes.addressof(bf)) == 0
    qf = qc.qp_frame(t, (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr), d_cu_qp.ptr, d_tu_qp_c.ptr,
                     [tabs[n].ptr for n in qc.TABLES], t.tw)
    assert dev.vvc355_deblock_qp_rec_pass(None, up(np.frombuffer(bytes(qf), np.uint8)).ptr, ctypes.addressof(qf)) == 0
    pitched = [batch.to_pitched(pl) for pl in planes]
    d_planes = [up(pl) for pl in pitched]
    d_dbp = up(dbp)
    frames = []
    for vertical in (1, 0):
        f = qc.deblock_frame(t, vertical, [d.ptr for d in d_planes], [pl.shape[1] * 2 for pl in pitched], lambda n: tabs[n].ptr,
                             [tabs[n].ptr for n in qc.TABLES], d_dbp.ptr)
        frames.append(f)
        dev.vvc355_deblock_frame_pass(None, qc.BD, up(np.frombuffer(bytes(f), np.uint8)).ptr, ctypes.addressof(f))
    dev.vvc355_stream_sync(None)
    for c in range(3):
        got = d_planes[c].to_host(np.uint16, pitched[c].shape)[:, :dims[c][0]]
        bad = np.argwhere(got != want[c])
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at {bad[0].tolist()}"

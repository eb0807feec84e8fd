"""GPU parity of the CIIP stage driver (vvc355_ciip_frame_pass): the job array the builder kernel writes from the decoder's tables and one
record per combined inter / intra coding unit against the restatement in ciip_frame_cases.py, the scratch buffer and the planes against
the oracle's orc_bipred_block run on the expected jobs, the VVC355_RECON_CIIP commands the builder completes (region address and the
intra weight of ciip_derive_intra_weight) against the numpy walk — and, end to end, a mixed picture through vvc355_ciip_frame_pass and
vvc355_recon_frame_pass against the oracle's reconstruction."""
import ctypes

import numpy as np
import pytest

import bipred_cases as bc
import ciip_frame_cases as cc
import recon_cases
from conftest import P
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu


def assert_jobs_equal(got, exp, what):
    for name in exp.dtype.names:
        bad = np.nonzero(np.any((got[name] != exp[name]).reshape(len(exp), -1), axis=1))[0]
        assert len(bad) == 0, f"{what}: field {name} differs in {len(bad)} jobs, first {bad[0]}: {got[name][bad[0]]} != {exp[name][bad[0]]}"


def assert_cmds_equal(got, exp, uploaded, what):
    bad = np.nonzero((got["resid"] != exp["resid"]) | (got["joint"] != exp["joint"]))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} commands differ in resid / joint, first {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"
    # every other byte is the upload's
    g, u = got.copy(), uploaded.copy()
    g["resid"], g["joint"], u["resid"], u["joint"] = 0, 0, 0, 0
    assert g.tobytes() == u.tobytes(), f"{what}: bytes outside resid / joint changed"
    same = (exp["resid"] == uploaded["resid"]) & (exp["joint"] == uploaded["joint"])
    assert got[same].tobytes() == uploaded[same].tobytes()


def check_outputs(run, want_jobs, want_scratch, want_planes, sentinel, what):
    p = run.p
    assert_jobs_equal(run.jobs(), run.expected_jobs(), what)
    assert np.array_equal(want_jobs["w"], run.expected_jobs()["w"])
    got = run.scratch()
    bad = np.nonzero(got != want_scratch)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} scratch pixels differ, first at {bad[0]}"
    inside = cc.region_mask(p, run.n_jobs, run.scratch_len)
    assert (~inside).any() and np.all(want_scratch[~inside] == sentinel) and (want_scratch[inside] != sentinel).mean() > 0.9
    for c in range(3):
        got = run.plane(c)
        bad = np.argwhere(got != want_planes[c])
        assert len(bad) == 0, f"{what}: component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"
        written = cc.plane_mask(p, c, run.n_jobs, run.scratch_len) if c else np.zeros(got.shape, bool)
        assert np.all(want_planes[c][~written] == sentinel)
        if written.any():
            assert (want_planes[c][written] != sentinel).mean() > 0.9


@pytest.mark.parametrize("case", range(len(cc.CASES)))
def test_ciip_frame_pass(dev, orc, case):
    bd = cc.CASES[case][0]
    p = cc.case_picture(case)
    rng = np.random.default_rng(0xC11B + case)
    dims, refs, lut = cc.pictures(rng, p, bd)
    sentinel = (1 << bd) // 3
    want_jobs, want_scratch, want_planes = cc.oracle_run(orc, p, bd, dims, refs, lut, sentinel)
    run = cc.DeviceRun(dev, p, bd, dims, refs, lut, sentinel)
    assert run.run() == 0
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    check_outputs(run, want_jobs, want_scratch, want_planes, sentinel, f"case {case}")
    assert_cmds_equal(run.cmds(), cc.expect_cmds(p, run.d_scratch.ptr), p.cmds, f"case {case}")


def test_malformed_records_are_rejected_and_change_nothing_else(dev, orc):
    bd = cc.CASES[0][0]
    p = cc.case_picture(0)
    q, where = cc.with_malformed(p)                      # (also puts ref_idx 16 into one background entry of the shared MvField table)
    rng = np.random.default_rng(0xC11B)
    dims, refs, lut = cc.pictures(rng, p, bd)
    sentinel = (1 << bd) // 3
    runs = {}
    for name, pic in (("valid", p), ("mixed", q)):
        want = cc.oracle_run(orc, pic, bd, dims, refs, lut, sentinel)
        run = cc.DeviceRun(dev, pic, bd, dims, refs, lut, sentinel)
        assert run.run() == 0
        dev.vvc355_stream_sync(None)
        assert dev.vvc355_last_error() == 0
        check_outputs(run, *want, sentinel, name)
        assert_cmds_equal(run.cmds(), cc.expect_cmds(pic, run.d_scratch.ptr), pic.cmds, name)
        runs[name] = run
    a, b = runs["valid"], runs["mixed"]
    # the rejected records' slots predict nothing ...
    jb = b.jobs()
    bad = np.zeros(len(q.cus), bool)
    bad[list(where.values())] = True
    for i in np.nonzero(bad)[0]:
        lo = int(q.cus[i]["first_job"])
        hi = int(q.cus[i + 1]["first_job"]) if i + 1 < len(q.cus) else q.n_jobs
        assert hi > lo and not jb[lo:hi].view(np.uint8).any(), i
    # ... and the valid units' output is the run's without them: the same regions (at their own offsets), the same planes, the same patches
    sa, sb = a.scratch(), b.scratch()
    for cu_a, cu_b in zip(p.cus, q.cus[~bad]):
        assert tuple(cu_a[n] for n in ("x0", "y0", "cb_width", "cb_height")) == tuple(cu_b[n] for n in ("x0", "y0", "cb_width", "cb_height"))
        n = cc.region_len(int(cu_a["cb_width"]), int(cu_a["cb_height"]), p.hs, p.vs, p.chroma)
        assert np.array_equal(sa[int(cu_a["scratch_off"]):int(cu_a["scratch_off"]) + n], sb[int(cu_b["scratch_off"]):int(cu_b["scratch_off"]) + n])
    for c in range(3):
        assert np.array_equal(a.plane(c), b.plane(c))
    ca, cb = a.cmds(), b.cmds()
    n = len(ca)
    patched = ca["resid"] != p.cmds["resid"]
    assert patched.any() and np.array_equal(ca["joint"], cb["joint"][:n]) and np.array_equal(cb["resid"][:n] != q.cmds["resid"][:n], patched)
    assert cb[n:].tobytes() == q.cmds[n:].tobytes()


def test_prediction_only_without_a_command_array(dev, orc):
    case = 2
    bd = cc.CASES[case][0]
    p = cc.case_picture(case)
    rng = np.random.default_rng(0xC11B + case)
    dims, refs, lut = cc.pictures(rng, p, bd)
    sentinel = (1 << bd) // 3
    want = cc.oracle_run(orc, p, bd, dims, refs, lut, sentinel)
    run = cc.DeviceRun(dev, p, bd, dims, refs, lut, sentinel, with_cmds=False)
    assert run.frame.cmds == 0 and run.frame.slice_idx == 0 and run.frame.ctb_to_col_bd == 0 and run.frame.ctb_to_row_bd == 0
    assert run.run() == 0
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    check_outputs(run, *want, sentinel, "cmds = 0")


def test_ciip_frame_pass_captured_in_a_graph(dev, orc):
    """Builder + prediction recorded once on a stream (both read their descriptors through device addresses) and replayed."""
    case = 3
    bd = cc.CASES[case][0]
    p = cc.case_picture(case)
    rng = np.random.default_rng(0xC11B + case)
    dims, refs, lut = cc.pictures(rng, p, bd)
    sentinel = (1 << bd) // 3
    want = cc.oracle_run(orc, p, bd, dims, refs, lut, sentinel)
    run = cc.DeviceRun(dev, p, bd, dims, refs, lut, sentinel)
    s = dev.vvc355_stream_create()
    dev.vvc355_graph_begin(s)
    assert run.run(s) == 0
    g = dev.vvc355_graph_end(s)
    dev.vvc355_stream_sync(s)
    assert np.all(run.scratch() == sentinel)             # recorded, not run
    dev.vvc355_graph_launch(g, s)
    dev.vvc355_stream_sync(s)
    assert dev.vvc355_last_error() == 0
    check_outputs(run, *want, sentinel, "graph")
    assert_cmds_equal(run.cmds(), cc.expect_cmds(p, run.d_scratch.ptr), p.cmds, "graph")
    dev.vvc355_graph_destroy(g)
    dev.vvc355_stream_destroy(s)


def test_ciip_then_recon_matches_the_oracle_reconstruction(dev, orc):
    """10 bit, 4:2:0, CTU 64, 256x192: intra, inter and CIIP units, two slices, tiles, LMCS (forward map on slice 0's inter part, chroma
    residual scaling in the walk).  The device gets the commands with resid = 0 and joint = 0 in every CIIP command; the oracle walks
    commands bound to host scratch that orc_bipred_block filled, carrying the numpy weights."""
    orc.orc_recon_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.ReconFrame)]
    orc.orc_recon_frame_pass.restype = None
    work, p = cc.e2e_work()
    bd, isz, hs, vs = p.bd, p.isz, p.hs, p.vs
    rng = np.random.default_rng(0xC11BE2E)
    dims, refs, lut = cc.pictures(rng, p, bd)
    planes = [bc.smooth_picture(rng, ph, pw, bd, scale=16) for (pw, ph) in dims]
    resid = rng.integers(-(1 << (bd - 3)), 1 << (bd - 3), size=max(1, work.resid_len)).astype(np.int32)
    model = recon_cases.ReconWork.lmcs_model(np.random.default_rng(0x1A5C + bd), bd)
    is_ciip = work.cmds["kind"] == abi.RECON_CIIP
    weights = cc.unit_weights(p)

    # ---- oracle: the inter parts into host scratch, then the walk
    scratch = np.zeros(p.scratch_len, planes[0].dtype)
    want = [pl.copy() for pl in planes]
    h_jobs = cc.expect_jobs(p, lambda c: (want[c].ctypes.data, dims[c][0] * isz), lambda l, r, c: (refs[l][r][c].ctypes.data, dims[c][0] * isz),
                            scratch.ctypes.data, lut.ctypes.data)
    assert np.all(h_jobs["w"] > 0) and np.all(h_jobs["dst"] >= scratch.ctypes.data) and np.all(h_jobs["dst"] < scratch.ctypes.data + scratch.nbytes)
    cc.call(orc.orc_bipred_block, bd, h_jobs)
    hc = work.bind(resid.ctypes.data, scratch.ctypes.data, isz)
    for u, cu in enumerate(p.cus):
        hc["joint"][cu["cmd"]] = weights[u]
    assert np.array_equal(hc[is_ciip], cc.expect_cmds(p, scratch.ctypes.data)[is_ciip])
    hf = work.frame([P(pl) for pl in want], [d[0] * isz for d in dims], hc.ctypes.data, work.ctus.ctypes.data, work.order.ctypes.data, 0,
                    work.slice_idx.ctypes.data, work.col_bd.ctypes.data, work.row_bd.ctypes.data, lmcs_ptr=ctypes.addressof(model))
    orc.orc_recon_frame_pass(bd, ctypes.byref(hf))

    # ---- device: commands uploaded with resid = 0, joint = 0 in the CIIP commands
    pitched = [batch.to_pitched(pl) for pl in planes]
    d_planes = [batch.DeviceBuffer.from_host(pl) for pl in pitched]
    pitches = [pl.shape[1] * isz for pl in pitched]
    d_res = batch.DeviceBuffer.from_host(resid)
    dcmd = work.bind(d_res.ptr, 0, isz)
    dcmd["resid"][is_ciip] = 0
    dcmd["joint"][is_ciip] = 0
    d_cmds, d_ctus, d_order = (batch.DeviceBuffer.from_host(a) for a in (dcmd.view(np.uint8), work.ctus.view(np.uint8), work.order))
    d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(work.ncx * work.ncy))
    d_slice, d_col, d_row = (batch.DeviceBuffer.from_host(a) for a in (work.slice_idx, work.col_bd, work.row_bd))
    d_model = batch.DeviceBuffer.from_host(np.frombuffer(bytes(model), np.uint8))
    d_ref = [[[batch.DeviceBuffer.from_host(batch.to_pitched(refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
    d_reft = batch.DeviceBuffer.from_host(np.frombuffer(bytes(cc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], pitches)), np.uint8))
    d_mvf, d_sl, d_lut = batch.DeviceBuffer.from_host(p.mvf.view(np.uint8)), batch.DeviceBuffer.from_host(np.frombuffer(bytes(p.slices), np.uint8)), batch.DeviceBuffer.from_host(lut)
    d_cus = batch.DeviceBuffer.from_host(p.cus.view(np.uint8))
    d_jobs = batch.DeviceBuffer(p.n_jobs * cc.BIPRED_JOB_DT.itemsize)
    d_scratch = batch.DeviceBuffer.from_host(np.zeros(p.scratch_len, planes[0].dtype))
    cf = p.frame(p.pic([b.ptr for b in d_planes], pitches, d_mvf.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr), d_cus.ptr, d_jobs.ptr, d_scratch.ptr, d_cmds.ptr,
                 d_slice.ptr, d_col.ptr, d_row.ptr)
    rf = work.frame([b.ptr for b in d_planes], pitches, d_cmds.ptr, d_ctus.ptr, d_order.ptr, d_state.ptr, d_slice.ptr, d_col.ptr, d_row.ptr, lmcs_ptr=d_model.ptr)
    d_cf, d_rf = (batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8)) for f in (cf, rf))
    assert dev.vvc355_ciip_frame_pass(None, bd, d_cf.ptr, ctypes.addressof(cf)) == 0
    dev.vvc355_recon_frame_pass(None, bd, d_rf.ptr, ctypes.addressof(rf))
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    assert np.array_equal(d_scratch.to_host(scratch.dtype, scratch.shape), scratch)
    for c in range(3):
        got = d_planes[c].to_host(pitched[c].dtype, pitched[c].shape)[:, :dims[c][0]]
        bad = np.argwhere(got != want[c])
        assert len(bad) == 0, f"component {c}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"
    assert sum(int((want[c] != planes[c]).sum()) for c in range(3)) > 256 * 192 // 4
    assert is_ciip.sum() >= 60 and len(np.unique(weights)) == 3

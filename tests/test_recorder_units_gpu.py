"""The unit entry of the recorder on the device: what vvc355_rec_ctu_units / vvc355_rec_units return is uploaded as it is and run through
the existing passes, and the result is compared with the oracle on inputs derived in numpy (tests/recorder_units_cases.py).

  CIIP pictures   three pictures (8 / 10 / 12 bit) with CIIP units: vvc355_ciip_frame_pass on the recorder's vvc355_ciip_cu list and
                  command array, the TB record passes, vvc355_lmcs_vpdu_scale_pass where chroma residual scaling is on,
                  vvc355_recon_frame_pass.  Oracle: orc_bipred_block on ciip_frame_cases.expect_jobs, the transform side of
                  ref_recon_cases.oracle_side, orc_recon_frame_pass on the extended derive()'s commands.  Planes whole, sentinels in the pitch padding.
  unit lists      cu / tu records and sidecars through vvc355_deblock_bs_rec_pass and vvc355_deblock_qp_rec_pass against orc_deblock_bs_pass on
                  tables painted from the units and against the painted QP tables; two pictures, one at CTU 128.
  motion lists    the vvc355_mvf_unit list through vvc355_mvf_unit_pass: every byte of the MvField table and of the affine records against
                  the numpy of mvf_unit_cases applied to the units.

The recorded picture on the device (RecordedCiip) and the chained oracle (ciip_oracle, inter_oracle) are tests/recorder_chain_cases.py's.
Before any launch the recorder's output is compared with the expectation (what tests/test_recorder_units_cpu.py asserts) and the ticket
order is checked by vvc355_recon_order_check: a malformed order makes the walk wait forever, so nothing unchecked reaches the device."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import bs_cases
import bs_rec_cases as brc
import mvf_unit_cases as mu
import picture_cases as pcs
import qp_rec_cases as qc
import recorder_units_cases as uc
import recorder_chain_cases as ch
import ref_recon_cases as rc
from ffvvc_amd import abi, batch
from recorder_chain_cases import RecordedCiip, ciip_oracle, inter_oracle

pytestmark = pytest.mark.gpu

_derived = {}


def _listed(name):
    if name not in _derived:
        pic = uc.picture(name) if name in uc.picture_names() else uc.units_picture(name)
        _derived[name] = (pic, uc.derive(pic))
    return _derived[name]


# ---------------------------------------------------------------------------------------------------------------- CIIP pictures

@pytest.mark.parametrize("name", uc.GPU_CIIP)
def test_ciip_pictures_reproduce_the_oracle(dev, orc, name):
    pic, d = _listed(name)
    assert pic.bd == {"U1": 8, "U5": 10, "U2": 12}[name]
    r = RecordedCiip(dev, pic, d)
    want = ciip_oracle(orc, pic, d, uc.expect_units(pic, d), r.refs, r.lut, r.dims)
    r.run_entries()
    got = r.result()
    bad = rc.first_difference(want[:3 if pic.idc else 1], got[:3 if pic.idc else 1])
    assert bad is None, f"{name}: {bad}"
    assert any(not np.array_equal(w, p) for w, p in zip(want, pic.planes))


# ---------------------------------------------------------------------------------------------------------------- unit lists

def bs_tables(pic, lfase=1, lfate=0):
    """A bs_cases.BsTables whose side tables are painted from the picture's units (the reference's table setters, one call site per record
    of INTEGRATION.md): coding-unit tables and MvField from the luma-tree units, transform-unit tables per tree."""
    t = bs_cases.BsTables.__new__(bs_cases.BsTables)
    g = uc.geometry(pic)
    t.width, t.height, t.ctb_log2, t.cw, t.ch, t.tw, t.th = pic.width, pic.height, pic.ctb_log2, g.cw, g.ch, g.tw, g.th
    t.lfase, t.lfate, t.hs, t.vs = lfase, lfate, pic.hs, pic.vs
    for n in ("cbf0", "cbf1", "cbf2", "joint", "pcm0", "pcm1", "tbw0", "tbw1", "tbh0", "tbh1", "cbw", "cbh", "msf", "iaf"):
        setattr(t, n, np.zeros((t.th, t.tw), np.uint8))
    for n in ("tbx0", "tbx1", "tby0", "tby1", "cbx", "cby"):
        setattr(t, n, np.zeros((t.th, t.tw), np.int32))
    t.mvf = np.ascontiguousarray(uc.paint_mvf(pic, np.zeros((t.th, t.tw), mu.MVF_DT))).view(np.dtype(abi.MvField)).reshape(t.th, t.tw)
    t.mvf["ref_idx"] = np.maximum(t.mvf["ref_idx"], 0)             # the unused list's index is never read; the tables keep it in range
    t.slice_idx, t.col_bd, t.row_bd = pic.slice_idx, pic.col_bd, pic.row_bd
    t.ref_poc = np.random.default_rng(uc.SEED).choice(np.array([0, 4, 8], np.int32), size=(len(pic.slices), 2, 32)).astype(np.int32)
    for ctu in pic.ctus:
        for cu in ctu:
            if cu["tree_type"] != 2:
                s = np.s_[cu["y0"] // 4:(cu["y0"] + cu["h"]) // 4, cu["x0"] // 4:(cu["x0"] + cu["w"]) // 4]
                t.cbx[s], t.cby[s], t.cbw[s], t.cbh[s] = cu["x0"], cu["y0"], cu["w"], cu["h"]
                if "pu" in cu:
                    t.msf[s], t.iaf[s] = cu["pu"]["msf"], cu["pu"]["kind"] == mu.AFFINE
            for tree in range(int(cu["tree_type"] == 2), 1 + int(cu["tree_type"] != 1)):
                for tu in cu["tus"]:
                    s = t._fill_tu(tree, tu["x0"], tu["y0"], tu["w"], tu["h"], tree)
                    if tree:
                        t.cbf1[s], t.cbf2[s], t.joint[s] = tu["coded"][1], tu["coded"][2], tu["joint"]
                    else:
                        t.cbf0[s] = tu["coded"][0]
    assert np.all(t.tbw0 > 0) and np.all(t.tbw1 > 0) and np.all(t.cbw > 0), "the units do not cover the picture"
    for name in t.OUT:
        setattr(t, name, np.full((t.th, t.tw), 0xEE, np.uint8))
    return t


def run_bs_rec(dev, t, u):
    """vvc355_deblock_bs_rec_pass on the recorder's lists and the uploaded MvField table, outputs pre-filled with 0xEE."""
    sentinel = np.full((t.th, t.tw), 0xEE, np.uint8)
    bufs = {name: batch.DeviceBuffer.from_host(sentinel) for name in t.OUT + brc.TB_C}
    for name in ("mvf", "ref_poc", "slice_idx", "col_bd", "row_bd"):
        a = getattr(t, name)
        bufs[name] = batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a)
    d = [batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a) for a in (u.cu, u.first_cu, u.tu, u.first_tu)]
    f = brc.rec_frame(t, (d[0].ptr, len(u.cu), d[1].ptr), (d[2].ptr, len(u.tu), d[3].ptr), lambda name: bufs[name].ptr)
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))
    ret = dev.vvc355_deblock_bs_rec_pass(None, d_f.ptr, ctypes.addressof(f))
    assert ret == 0, f"vvc355_deblock_bs_rec_pass refused the frame: {ret}"
    dev.vvc355_stream_sync(None)
    return {name: bufs[name].to_host(np.uint8, (t.th, t.tw)) for name in t.OUT + brc.TB_C}


@pytest.mark.parametrize("name", uc.GPU_UNITS)
def test_unit_lists_give_the_deblocking_tables(dev, orc, name):
    pic, d = _listed(name)
    assert pic.ctb_log2 == {"V64": 6, "V128": 7}[name] and pic.idc
    o = ch.checked_record(dev, pic, d)
    u = o.u
    t = bs_tables(pic)
    want = brc.expected(t, bs_cases.run_oracle(orc, t))
    got = run_bs_rec(dev, t, u)
    bad = brc.mismatches(got, want, t.OUT + brc.TB_C)
    assert not bad, f"{name}: " + "; ".join(bad)
    assert any(want[n].any() for n in ("bs00", "bs10", "bs01", "bs11"))
    p = qc.Pic(g=uc.geometry(pic), cu=u.cu, tu=u.tu, cu_first=u.first_cu, tu_first=u.first_tu, cu_qp=u.cu_qp, tu_qp_c=np.ascontiguousarray(u.tu_qp_c))
    bad = qc.mismatches(qc.run_device(dev, p), uc.paint_qp(pic), p.g)
    assert not bad, f"{name}: " + "; ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- motion lists

@pytest.mark.parametrize("name", ["U2", "U5"])
def test_motion_lists_give_the_mvfield_table(dev, name):
    pic, d = _listed(name)
    o = ch.checked_record(dev, pic, d)
    u = o.u
    assert len(u.affine) > 2 and (u.mvf["kind"] == mu.GPM).any() and (u.mvf["kind"] == mu.AFFINE).any()
    g = mu.Geo(pic.width, pic.height, pic.ctb_log2)
    table, cus = mu.sentinel_table(g, g.tw + 3), u.affine.copy()
    t_want, c_want = table.copy(), cus.copy()
    uc.paint_mvf(pic, t_want[:g.th, :g.tw], c_want)
    t_got, c_got, ret = mu.run_device(dev, g, u.mvf, u.first_mvf, table, cus)
    assert ret == 0
    assert not mu.table_mismatch(t_got, t_want), mu.table_mismatch(t_got, t_want)
    assert not mu.cus_mismatch(c_got, c_want), mu.cus_mismatch(c_got, c_want)
    assert c_want["prof_flags"].any() and c_want["diff_mv"].any()


# ---------------------------------------------------------------------------------------------------------------- one whole picture

def _whole_picture(dev, orc, pic, d, order):
    """The picture through vvc355_mvf_unit_pass and ONE vvc355_picture_pass, every list the recorder's: (tables and planes got, the same wanted)."""
    import ref_pass_cases as pc
    from test_picture_gpu import _filter_stages
    from test_ref_passes_gpu import Device, _download
    bd, isz, g = pic.bd, pic.isz, mu.Geo(pic.width, pic.height, pic.ctb_log2)
    rng = np.random.default_rng([uc.SEED, 0xA11])
    dv = Device(dev)
    e = uc.expect_units(pic, d)
    # ---- device: the MvField table and the affine records' PROF fields from the motion records, before the picture
    d_mvf = dv.up(np.full((g.th, g.tw, 24), 0xEE, np.uint8))
    r = RecordedCiip(dev, pic, d, order=order, d_mvf=d_mvf)
    o, u, k = r.o, r.o.u, r.k
    mf, inter_stages = r.motion_stages(d_mvf)
    assert dev.vvc355_mvf_unit_pass(None, mf[0], ctypes.addressof(mf[1])) == 0
    st = dict(r.stages, **inter_stages)
    planes_ptr, strides = [b.ptr for b in r.d_planes], r.strides
    # the deblocking side: the recorder's cu / tu lists and sidecars, the table the motion pass wrote
    t = bs_tables(pic, 0, 0)
    dbp = (2 * rng.integers(-12, 13, size=(t.cw * t.ch, 6))).astype(np.int8)
    rec = qc.Pic(g=t, cu=u.cu, tu=u.tu, cu_first=u.first_cu, tu_first=u.first_tu, cu_qp=u.cu_qp, tu_qp_c=np.ascontiguousarray(u.tu_qp_c))
    tabs = {nm: k.up(np.full((t.th, t.tw), 0xEE, np.uint8)) for nm in t.OUT + brc.TB_C + qc.TABLES}
    tabs.update(mvf=d_mvf, ref_poc=k.up(t.ref_poc), slice_idx=r.d_maps[0], col_bd=r.d_maps[1], row_bd=r.d_maps[2], dbp=k.up(dbp))
    addr = lambda nm: tabs[nm].ptr                                                        # noqa: E731
    cu_arg, tu_arg = (k.up(u.cu).ptr, len(u.cu), k.up(u.first_cu).ptr), (k.up(u.tu).ptr, len(u.tu), k.up(u.first_tu).ptr)
    inv_lut = rng.integers(0, 1 << bd, size=1 << bd, dtype=np.int64).astype(pic.planes[0].dtype)
    used = np.array([sl[1] for sl in pic.slices], np.uint8)
    shape = SimpleNamespace(width=pic.width, height=pic.height, cw=pic.ncx, ch=pic.ncy, n_slices=len(pic.slices), ctb_log2=pic.ctb_log2, pitch=strides[0])
    dp = pc._finish_deblock("whole", bd, 3, t, None, uc.paint_qp(pic), dbp, None, rec)
    fp = pc.draw_filter("whole", rng, bd, (pic.hs, pic.vs), 3, t.ctb_log2, None, dp.n_slices, True, (0, 0), t=t, planes=False)
    st.update(bs_rec=k.frame(brc.rec_frame(t, cu_arg, tu_arg, addr)),
              qp_rec=k.frame(qc.qp_frame(t, cu_arg, tu_arg, k.up(u.cu_qp).ptr, k.up(rec.tu_qp_c).ptr, [tabs[nm].ptr for nm in qc.TABLES], t.tw)),
              lmcs=k.frame(pcs.lmcs_frame(shape, planes_ptr[0], k.up(inv_lut).ptr, r.d_maps[0].ptr, k.up(used).ptr)),
              deblock_v=k.frame(pc.deblock_frame(dp, 1, planes_ptr, strides, addr)), deblock_h=k.frame(pc.deblock_frame(dp, 0, planes_ptr, strides, addr)))
    more, work, out = _filter_stages(dv, fp, r.d_planes, r.host_planes)
    st.update(more)
    assert set(st) == {"inter", "affine", "gpm", "ciip", "intra_tb", "inter_tb", "ts_tb", "lmcs_scale", "bs_rec", "qp_rec", "recon", "lmcs",
                       "deblock_v", "deblock_h", "sao", "alf"}
    ret = pcs.run(dev, None, bd, pcs.picture(st, alf_work=work, recon_tables=(o.ctus, o.order)))
    assert ret == 0, f"vvc355_picture_pass refused the picture: stage / code {pcs.decode(ret)}"
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    got = {nm: tabs[nm].to_host(np.uint8, (t.th, t.tw)) for nm in t.OUT}
    got["h"] = r.result()
    got["sao"], got["alf"] = (_download(*out[s], pic.planes) for s in ("sao", "alf"))
    # ---- the chained oracle
    aff = e.affine.copy()
    mvf = uc.paint_mvf(pic, np.zeros((g.th, g.tw), mu.MVF_DT), aff)
    start = inter_oracle(orc, pic, e, mvf, aff, r.refs, r.lut, r.dims, r.p.slices, [np.ascontiguousarray(p).copy() for p in pic.planes])
    recon = ciip_oracle(orc, pic, d, e, r.refs, r.lut, r.dims, start=start)
    mask = pcs.lmcs_mask(pic.width, pic.height, pic.ctb_log2, pic.slice_idx, used)
    dp.planes = [np.where(mask, inv_lut[recon[0]], recon[0]).astype(recon[0].dtype), recon[1], recon[2]]
    want = pc.run_deblock(orc, "orc", dp)
    want["sao"] = pc.run_filter(orc, "orc", fp, "sao", want["h"])
    want["alf"] = pc.run_filter(orc, "orc", fp, "alf", want["sao"])
    return got, want, dp, (start, recon)


def test_one_whole_picture_from_the_recorder(dev, orc):
    """vvc355_mvf_unit_pass, then one vvc355_picture_pass with every stage the recorder feeds (the four kinds of inter units, the three TB
    passes around the scale pass, the deblocking tables from the unit records, the walk) plus inverse LMCS and drawn deblocking, SAO and
    ALF parameters, against the chained oracle passes; once more with the CTUs recorded in a shuffled order, with equal output."""
    import ref_pass_cases as pc
    pic, d = _listed("V64")
    runs = []
    for order in (None, np.random.default_rng(0x0DE3).permutation(len(pic.ctus))):
        got, want, dp, (start, recon) = _whole_picture(dev, orc, pic, d, order)
        lines = pc.table_differences(dp, want, got, label="oracle")
        for s in ("h", "sao", "alf"):
            lines += pc.plane_differences("whole picture", s, want[s], got[s], label="oracle")
        assert not lines, "\n".join(lines)
        assert all(np.any(a != b) for a, b in zip(start, pic.planes)) and all(np.any(a != b) for a, b in zip(recon, start))
        assert all(np.any(a != b) for a, b in zip(want["h"], dp.planes)) and all(np.any(a != b) for a, b in zip(want["alf"], want["sao"]))
        runs.append(got)
    for nm in runs[0]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0][nm], runs[1][nm])), f"{nm} differs between raster and shuffled recording"

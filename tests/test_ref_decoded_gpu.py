"""Whole decoded pictures on the device against tests/golden/ref_decoded.json: what the reference's picture chain followed by its own
deblocking, SAO and ALF callers left on the pictures of tests/ref_decoded_cases.py (W0-W9, Q0-Q2).  The test reads only the digests.

Every list is the recorder's (vvc355_rec_ctu_units + vvc355_rec_units, the filters' transform-unit records from vvc355_rec_deblock_units), compared with the expectation before any launch
(recorder_chain_cases.checked_record).  Per picture: vvc355_mvf_unit_pass into a table that starts as garbage, then ONE
vvc355_picture_pass with every stage on — tab_fill (the side tables from the cu / tu records), the inter / affine / GPM / CIIP stages, the
TB passes around the scale pass, RECON, inverse LMCS, bs_rec, qp_rec, both deblocking directions, SAO and ALF — in vvc355_recon_order's
ticket order, two pictures also in raster order.  Held to the digests: tab_dmvr_mvf, the ten bS / length tables, the QP tables, the planes
after H, after SAO and the final ones.  Every plane has sentinel bytes in its pitch padding and sentinel rows above and below, checked
afterwards.  Three pictures (one per bit depth) also go through the separate entries in INTEGRATION.md's order, which must leave what the
one call left.  On the final planes vvc355_pic_digest_pass and vvc355_pic_output_pass (with a conformance window) must give what zlib /
binascii / numpy give on them.  On a mismatch the oracle chain runs the same picture and the message names the first differing stage."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import bs_cases
import bs_rec_cases as brc
import inter_tb_cases as tc
import mvf_unit_cases as mu
import pic_digest_cases as pdc
import pic_output_cases as poc
import picture_cases as pcs
import qp_rec_cases as qc
import recorder_chain_cases as ch
import ref_decoded_cases as dc
import ref_pass_cases as ps
import ref_picture_cases as pc
import ref_recon_cases as rc
from ffvvc_amd import abi
from test_ref_picture_gpu import DevicePicture

pytestmark = pytest.mark.gpu
SIDE = [n for n in bs_cases.BsTables.FILLED if n != "mvf"]


@pytest.fixture(scope="module")
def golden():
    return dc.load_golden()


class DecodedPicture(DevicePicture):
    """test_ref_picture_gpu's picture with the filter half on the same planes: frames of tab_fill, bs_rec, qp_rec, deblock_v / _h, sao, alf."""

    def __init__(self, dev, orc, pic, raster=False):
        super().__init__(dev, pic, raster)
        c = self.c = dc.case(orc, pic)
        r, k, u = self.r, self.r.k, self.r.o.u
        dp, fp = c.dp_orc, c.fp
        t = self.t = dp.t
        chroma = c.n_comp == 3
        luma_out = ("bs00", "bs10", "p0", "p1", "q0", "q1")
        tabs = self.tabs = {n: k.up(np.full((t.th, t.tw), 0xEE if chroma or n in luma_out else 0, np.uint8)) for n in t.OUT}
        for n in brc.TB_C + qc.TABLES:
            tabs[n] = k.up(np.full((t.th, t.tw), 0xEE, np.uint8))
        tabs["mvf"] = self.d_mvf
        for n in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
            tabs[n] = k.up(getattr(t, n))
        tabs["dbp"] = k.up(c.dbp)
        addr = lambda n: tabs[n].ptr          # noqa: E731
        d_cu, d_cu_first, d_tu, d_tu_first, d_cu_qp, d_tu_qp_c = (k.up(a) for a in (u.cu, u.first_cu, u.tud, u.first_tud, u.cu_qp, u.tud_qp_c))
        cu_arg, tu_arg = (d_cu.ptr, len(u.cu), d_cu_first.ptr), (d_tu.ptr, len(u.tud), d_tu_first.ptr)
        self.side = {n: k.up(np.zeros_like(getattr(t, n))) for n in SIDE}
        planes_ptr, strides = [b.ptr for b in r.d_planes], r.strides
        st = self.stages
        st["tab_fill"] = k.frame(t.fill_frame(d_cu.ptr, d_tu.ptr, 0, (len(u.cu), len(u.tud), 0), lambda n: self.side[n].ptr if n in self.side else 0,
                                              (d_cu_first.ptr, d_tu_first.ptr, 0)))
        st["bs_rec"] = k.frame(brc.rec_frame(t, cu_arg, tu_arg, addr, c.n_comp, tb_c=chroma))
        st["qp_rec"] = k.frame(qc.qp_frame(t, cu_arg, tu_arg if chroma else (0, 0, 0), d_cu_qp.ptr, d_tu_qp_c.ptr if chroma else 0,
                                           [tabs[n].ptr if chroma or n == "qp_y" else 0 for n in qc.TABLES], t.tw, c.n_comp))
        st["deblock_v"] = k.frame(ps.deblock_frame(dp, 1, planes_ptr, strides, addr))
        st["deblock_h"] = k.frame(ps.deblock_frame(dp, 0, planes_ptr, strides, addr))
        ftabs = {"sao": k.up(fp.sao), "alf": k.up(fp.alf), "slice_idx": tabs["slice_idx"], "col_bd": tabs["col_bd"], "row_bd": tabs["row_bd"]}
        ftabs["slices"] = k.up(np.frombuffer(bytes(ps.alf_slices(fp, [k.up(a).ptr for a in fp.aps])), np.uint8))
        self.out_host = [tc.pitched(np.full(p.shape, 0x21, p.dtype)) for p in pic.planes[:c.n_comp]]
        self.d_sao = [ch.GuardedPlane(k, h, 2) for h in self.out_host]
        self.d_alf = [ch.GuardedPlane(k, h, 2) for h in self.out_host]
        n = c.n_comp
        st["sao"] = k.frame(ps.sao_frame(fp, [b.ptr for b in self.d_sao], planes_ptr[:n], strides[:n], strides[:n], lambda name: ftabs[name].ptr))
        st["alf"] = k.frame(ps.alf_frame(fp, [b.ptr for b in self.d_alf], [b.ptr for b in self.d_sao], strides[:n], strides[:n], lambda name: ftabs[name].ptr))
        self.alf_work = k.up(np.zeros(dev.vvc355_alf_frame_work_bytes(t.cw * t.ch), np.uint8)).ptr

    def one_call(self):
        self.motion()
        ret = pcs.run(self.dev, None, self.pic.bd, pcs.picture(self.stages, alf_work=self.alf_work, recon_tables=(self.r.o.ctus, self.r.ticket)))
        assert ret == 0, f"vvc355_picture_pass refused the picture: stage / code {pcs.decode(ret)}"

    def entries(self):
        """The separate entries in INTEGRATION.md's order."""
        dev, st, bd = self.dev, self.stages, self.pic.bd
        at = lambda name: (st[name][0], ctypes.addressof(st[name][1]))          # noqa: E731
        self.motion()
        dev.vvc355_tab_fill_pass(None, *at("tab_fill"))
        self.prediction_and_reconstruction()
        self.inverse_lmcs()
        assert dev.vvc355_deblock_bs_rec_pass(None, *at("bs_rec")) == 0
        assert dev.vvc355_deblock_qp_rec_pass(None, *at("qp_rec")) == 0
        dev.vvc355_deblock_frame_pass(None, bd, *at("deblock_v"))
        dev.vvc355_deblock_frame_pass(None, bd, *at("deblock_h"))
        dev.vvc355_sao_frame_pass(None, bd, *at("sao"))
        dev.vvc355_alf_frame_pass(None, bd, *at("alf"), self.alf_work)

    def _guarded(self, bufs):
        out = []
        for c, (b, h, p) in enumerate(zip(bufs, self.out_host, self.pic.planes)):
            g = b.to_host(h.dtype, h.shape)
            assert np.array_equal(g[:, p.shape[1]:], h[:, p.shape[1]:]), f"component {c}: the pitch padding of an output plane was written"
            out.append(g[:, :p.shape[1]].copy())
        return out

    def outputs(self):
        """Everything the digests cover, downloaded: the result of ref_decoded_cases.run_oracle's second value plus dmvr and the side tables."""
        t, n = self.t, self.c.n_comp
        out = {"h": self.r.result()[:n]}                       # synchronises; guard rows and pitch padding of the picture's planes checked
        out["sao"], out["alf"] = self._guarded(self.d_sao), self._guarded(self.d_alf)
        for name in t.OUT:
            out[name] = self.tabs[name].to_host(np.uint8, (t.th, t.tw))
        for name in qc.TABLES:
            out[name] = self.tabs[name].to_host(np.int8, (t.th, t.tw))
        g = self.g
        out["dmvr"] = self.d_dmvr.to_host(np.uint8, (g.th, g.tw, 24)).view(mu.MVF_DT).reshape(g.th, g.tw)
        out["tbw1"], out["tbh1"] = (self.tabs[k].to_host(np.uint8, (t.th, t.tw)) for k in brc.TB_C)
        out["side"] = {k: self.side[k].to_host(getattr(t, k).dtype, getattr(t, k).shape) for k in SIDE}
        return out


def _digests(orc, pic, out):
    return dc.digests(orc, pic, SimpleNamespace(dmvr=out["dmvr"]), out)


def _held(orc, pic, golden, out):
    """The device's run against the reference's digests; the oracle chain names the first differing stage on a mismatch."""
    name = pic.name
    got = _digests(orc, pic, out)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name])
    bad = [k for k in got if got[k] != golden[name][k]]
    if bad:
        o, want = dc.run_oracle(orc, pic)
        lines = dc.differences(pic, dc.case(orc, pic).dp_orc, want, out, label="oracle", stages=dc.STAGES)
        if not np.array_equal(pc.mvf_bytes(o.dmvr), pc.mvf_bytes(out["dmvr"])):
            lines.insert(0, f"{name}: tab_dmvr_mvf differs from the oracle chain's")
        pytest.fail(f"{name}: {bad} do not hash to the reference's digests\n" + "\n".join(lines or ["the oracle chain agrees with the device: it no longer "
                    "reproduces the digests either (tests/test_ref_decoded_cpu.py)"]))


def _side_tables(p, out):
    """vvc355_tab_fill_pass on the recorder's records against orc_tab_fill_pass on the expected ones."""
    want = p.c.dp_orc.arrays
    chroma = p.c.n_comp == 3
    bad = [k for k in SIDE if (chroma or not k.endswith("1") and k not in ("cbf1", "cbf2", "joint")) and not np.array_equal(out["side"][k], want[k])]
    assert not bad, f"{p.pic.name}: side tables {bad} of the tab_fill stage differ from the oracle's"
    if chroma:
        assert np.array_equal(out["tbw1"], want["tbw1"]) and np.array_equal(out["tbh1"], want["tbh1"]), "tb_width_c / tb_height_c of the bs_rec stage"


def _digest_and_output(dev, p, final):
    """vvc355_pic_digest_pass and vvc355_pic_output_pass on the final planes in device memory."""
    pic, n = p.pic, p.c.n_comp
    bd, px = pic.bd, pic.isz
    dims = [(q.shape[1], q.shape[0]) for q in final]
    ptrs, strides = [b.ptr for b in p.d_alf], p.r.strides[:n]
    got = pdc.Run(dev, bd, dims, ptrs, strides).run()
    want = pdc.expected(final, bd)
    assert got == want, f"{pic.name}: vvc355_pic_digest_pass: {pdc.describe(got, want)}"
    # a conformance window: 2 chroma columns and 1 chroma row off the left / top, 3 and 2 off the right / bottom
    hs, vs = (pic.hs, pic.vs) if n == 3 else (0, 0)
    x0, y0, x1, y1 = 2 << hs, 1 << vs, pic.width - (3 << hs), pic.height - (2 << vs)
    win, src = [], []
    for c in range(n):
        sx, sy = (hs, vs) if c else (0, 0)
        cx0, cy0, cx1, cy1 = x0 >> sx, y0 >> sy, x1 >> sx, y1 >> sy
        win.append(np.ascontiguousarray(final[c][cy0:cy1, cx0:cx1]))
        src.append(ptrs[c] + cy0 * strides[c] + cx0 * px)
    cdims = [(w.shape[1], w.shape[0]) for w in win]
    for mode in ((abi.OUT_PLANAR, bd, False), (abi.OUT_SEMI, 16, True)) if n == 3 else ((abi.OUT_PLANAR, 16, False),):
        bad = poc.OutRun(dev, bd, cdims, src, strides, mode).run(win)
        assert not bad, f"{pic.name}: vvc355_pic_output_pass on the window ({x0}, {y0})-({x1}, {y1}): {bad}"


@pytest.mark.parametrize("name,raster", [(n, False) for n in dc.picture_names()] + [(n, True) for n in dc.RASTER_TOO])
def test_one_picture_pass_reproduces_the_decoded_reference(dev, orc, golden, name, raster):
    pic = dc.picture(name)
    p = DecodedPicture(dev, orc, pic, raster)
    assert set(p.stages) >= {"tab_fill", "inter", "affine", "gpm", "ciip", "recon", "lmcs", "bs_rec", "qp_rec", "deblock_v", "deblock_h", "sao", "alf"}
    assert ("lmcs_scale" in p.stages) == bool(pic.chroma_scale_flag) and set(p.stages) <= set(abi.PIC_STAGES)
    assert not raster or np.array_equal(p.r.ticket, np.sort(p.r.ticket))
    p.one_call()
    out = p.outputs()
    _held(orc, pic, golden, out)
    _side_tables(p, out)
    if not raster:
        _digest_and_output(dev, p, out["alf"])


@pytest.mark.parametrize("name", dc.ENTRIES_TOO)
def test_separate_entries_leave_what_the_one_call_leaves(dev, orc, golden, name):
    pic = dc.picture(name)
    a, b = DecodedPicture(dev, orc, pic), DecodedPicture(dev, orc, pic)
    a.one_call()
    b.entries()
    one, sep = a.outputs(), b.outputs()
    _held(orc, pic, golden, sep)
    for k in one:
        pairs = zip(one[k], sep[k]) if isinstance(one[k], list) else [(one[k][s], sep[k][s]) for s in one[k]] if isinstance(one[k], dict) else [(one[k], sep[k])]
        assert all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in pairs), f"{name}: {k} differs between the two ways"
    assert rc.sha(*one["alf"]) == rc.sha(*sep["alf"])

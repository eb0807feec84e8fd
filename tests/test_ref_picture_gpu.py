"""Inter prediction, reconstruction and inverse LMCS of whole pictures on the device against tests/golden/ref_picture.json: what the
reference's own three calls per CTU (ff_vvc_predict_inter, ff_vvc_reconstruct with ff_vvc_predict_ciip, ff_vvc_lmcs_filter) left on the
pictures W0-W9 of tests/ref_picture_cases.py.  The test reads only the digests.

Every list is the recorder's (vvc355_rec_ctu_units + vvc355_rec_units), uploaded as it is; before any launch it is compared with the
expectation and the ticket order is checked (recorder_chain_cases.checked_record).  Two kinds of run:

  entries   the separate entries in INTEGRATION.md's order: vvc355_mvf_unit_pass; vvc355_inter_frame_pass, vvc355_affine_frame_pass,
            vvc355_gpm_frame_pass; vvc355_ciip_frame_pass; the three TB record passes around vvc355_lmcs_vpdu_scale_pass;
            vvc355_recon_frame_pass — planes, dmvr_mvf and the scale table downloaded and held to the reconstruction digests;
            vvc355_lmcs_frame_pass — planes held to the final digests.
  picture   vvc355_mvf_unit_pass, then ONE vvc355_picture_pass with the same stages and the filter half off, held to the final digests (and
            dmvr, scale): W0-W9 in vvc355_recon_order's ticket order, two of them also in ascending raster order.

The planes start sentinel-filled, have sentinel bytes in the pitch padding and sentinel rows above and below, and are compared whole."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import mvf_unit_cases as mu
import picture_cases as pcs
import recorder_chain_cases as ch
import ref_picture_cases as pc
import ref_recon_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


class DevicePicture:
    """The picture recorded and uploaded; every stage's frame filled from the recorder's results."""

    def __init__(self, dev, pic, raster=False):
        i = pc.inputs(pic)
        self.dev, self.pic, self.d, self.n = dev, pic, i.d, i.n
        g = self.g = mu.Geo(pic.width, pic.height, pic.ctb_log2)
        k0 = pcs.Keep()
        self.d_mvf = k0.up(np.full((g.th, g.tw, 24), 0xEE, np.uint8))
        r = self.r = ch.RecordedCiip(dev, pic, i.d, d_mvf=self.d_mvf, ticket=i.d.order if raster else None, guard=2)
        k = r.k
        k.keep.append(k0)
        # tab_dmvr_mvf as the parser leaves it: a copy of the motion field, here of the table vvc355_mvf_unit_pass wrote (motion() copies it)
        self.d_dmvr = k.up(np.full((g.th, g.tw, 24), 0xDD, np.uint8))
        self.mvf_stage, inter_stages = r.motion_stages(self.d_mvf, self.d_dmvr.ptr)
        planes_ptr, strides = [b.ptr for b in r.d_planes], r.strides
        self.used = np.array([sl[1] for sl in pic.slices], np.uint8)
        shape = SimpleNamespace(width=pic.width, height=pic.height, cw=pic.ncx, ch=pic.ncy, n_slices=len(pic.slices), ctb_log2=pic.ctb_log2, pitch=strides[0])
        st = self.stages = dict(r.stages, **inter_stages)
        st.update(lmcs=k.frame(pcs.lmcs_frame(shape, planes_ptr[0], k.up(pic.inv_lut).ptr, r.d_maps[0].ptr, k.up(self.used).ptr)))

    def motion(self):
        assert self.dev.vvc355_mvf_unit_pass(None, self.mvf_stage[0], ctypes.addressof(self.mvf_stage[1])) == 0
        self.dev.vvc355_copy_async(None, self.d_dmvr.ptr, self.d_mvf.ptr, self.g.th * self.g.tw * 24)

    def prediction_and_reconstruction(self):
        dev, st, bd = self.dev, self.stages, self.pic.bd
        for name, fn in (("inter", dev.vvc355_inter_frame_pass), ("affine", dev.vvc355_affine_frame_pass), ("gpm", dev.vvc355_gpm_frame_pass)):
            fn(None, bd, st[name][0], ctypes.addressof(st[name][1]))
        self.r.run_entries()

    def inverse_lmcs(self):
        st = self.stages["lmcs"]
        assert self.dev.vvc355_lmcs_frame_pass(None, self.pic.bd, st[0], ctypes.addressof(st[1])) == 0

    def digests(self, prefix):
        """The digests of what is on the device now: planes (whole, the padding and the rows around them checked), dmvr, scale."""
        planes = self.r.result()[:self.n]
        g, d = self.g, self.d
        dmvr = self.d_dmvr.to_host(np.uint8, (g.th, g.tw, 24)).view(mu.MVF_DT).reshape(g.th, g.tw)
        table = self.r.d_table.to_host(np.int16, (d.tpic.uy, d.tpic.ux)) if self.r.scaled else None
        out = {f"{prefix}{c}": rc.sha(p) for c, p in enumerate(planes)}
        out.update(dmvr=rc.sha(pc.mvf_bytes(dmvr)), scale=rc.scale_digest(d, table))
        return out, planes


def _held(name, golden, got, keys):
    bad = sorted(k for k in keys if got[k] != golden[name][k])
    assert not bad, f"{name}: {bad} do not hash to the reference's digests (tests/test_ref_picture_cpu.py names the first sample where the library is built)"


@pytest.mark.parametrize("name", pc.picture_names())
def test_separate_entries_reproduce_the_reference(dev, golden, name):
    pic = pc.picture(name)
    assert golden[name]["inputs"] == pc.inputs_digest(pic), f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    p = DevicePicture(dev, pic)
    p.motion()
    p.prediction_and_reconstruction()
    got, recon = p.digests("r")
    _held(name, golden, got, [f"r{c}" for c in range(p.n)] + ["dmvr", "scale"])
    p.inverse_lmcs()
    got, final = p.digests("p")
    _held(name, golden, got, [f"p{c}" for c in range(p.n)] + ["dmvr", "scale"])
    assert np.array_equal(recon[0], final[0]) != bool(p.used.any())
    assert all(np.array_equal(a, b) for a, b in zip(recon[1:], final[1:]))


@pytest.mark.parametrize("name,raster", [(n, False) for n in pc.picture_names()] + [(n, True) for n in pc.RASTER_TOO])
def test_one_picture_pass_reproduces_the_reference(dev, golden, name, raster):
    pic = pc.picture(name)
    assert golden[name]["inputs"] == pc.inputs_digest(pic), f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    p = DevicePicture(dev, pic, raster)
    st = p.stages
    assert {"inter", "affine", "gpm", "ciip", "recon", "lmcs"} <= set(st) <= {"inter", "affine", "gpm", "ciip", "intra_tb", "inter_tb", "ts_tb", "lmcs_scale",
                                                                              "recon", "lmcs"}
    assert ("lmcs_scale" in st) == bool(pic.chroma_scale_flag)
    assert not raster or np.array_equal(p.r.ticket, np.sort(p.r.ticket))
    p.motion()
    ret = pcs.run(dev, None, pic.bd, pcs.picture(st, recon_tables=(p.r.o.ctus, p.r.ticket)))
    assert ret == 0, f"vvc355_picture_pass refused the picture: stage / code {pcs.decode(ret)}"
    got, _final = p.digests("p")
    _held(name, golden, got, [f"p{c}" for c in range(p.n)] + ["dmvr", "scale"])

"""GPU: the inter prediction stage drivers held to the reference's own digests (tests/golden/ref_inter.json: what ff_vvc_predict_inter and
ff_vvc_predict_ciip computed on the pictures of tests/ref_inter_cases.py), with no oracle in between, on pitched device planes:

* vvc355_inter_frame_pass: every plane and tab_dmvr_mvf (R0-R7);
* vvc355_affine_frame_pass (A0-A3) and vvc355_gpm_frame_pass (G0-G2): every plane;
* M0: the three drivers one after the other on the same planes, against the three reference entries in the same order;
* vvc355_ciip_frame_pass (I0-I4): the scratch, the planes (chroma of 2-wide blocks lands there) and the .joint bytes of the patched commands.
The 4:0:0 pictures run with chroma_format_idc 0.  Only the committed digests are read.  On a mismatch the oracle runs the same picture (it
reproduces the same digests, tests/test_ref_inter_cpu.py) and the message names the first differing sample and the unit that covers it."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import affine_gpm_cases as agc
import ciip_frame_cases as cc
import inter_frame_cases as ifc
import ref_inter_cases as ic
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return ic.load_golden()


def _up(a):
    a = np.ascontiguousarray(a)
    return batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a)


def _scratch(nbytes):
    return batch.DeviceBuffer(max(int(nbytes), 64))


def device_picture(dev, pic, stages="RAG"):
    """The picture's units of the given kinds through their stage drivers, in this order on the same sentinel-filled pitched planes:
    (planes, tab_dmvr_mvf)."""
    dt = ic.px(pic.bd)
    pitches = [batch.plane_pitch(d[0], pic.isz) for d in pic.dims]
    pitched = [batch.to_pitched(np.full((ph, pw), pic.sentinel, dt)) for (pw, ph) in pic.dims[:pic.n_comp]]
    d_dst = [_up(p) for p in pitched]
    d_ref = [[[_up(batch.to_pitched(pic.refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
    reft = agc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], [[pitches] * 2] * 2)
    d_reft, d_mvf, d_dmvr = _up(np.frombuffer(bytes(reft), np.uint8)), _up(pic.mvf), _up(pic.mvf)
    d_sl, d_lut = _up(np.frombuffer(bytes(pic.slices), np.uint8)), _up(pic.lut)
    d_pus, d_acu, d_gcu = (_up(a) if len(a) else _scratch(0) for a in (pic.pus, pic.aff, pic.gpm))
    d_jl, d_jc, d_rec = _scratch(pic.n_jobs * agc.BIPRED_JOB_DT.itemsize), _scratch(2 * pic.n_jobs * agc.BIPRED_JOB_DT.itemsize), _scratch(pic.n_jobs * 32)
    d_ajl, d_ajc = _scratch(pic.n_aff_jobs * agc.AFFINE_JOB_DT.itemsize), _scratch(pic.n_aff_chroma_jobs() * agc.BIPRED_JOB_DT.itemsize)
    d_gj = _scratch(pic.n_gpm_jobs * agc.GPM_JOB_DT.itemsize)
    f = pic.frame([b.ptr for b in d_dst] + [0] * (3 - pic.n_comp), pitches, d_mvf.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr, d_pus.ptr, d_jl.ptr, d_jc.ptr,
                  d_rec.ptr, d_dmvr.ptr)
    keep = []
    for kind in stages:
        if kind not in pic.kinds:
            continue
        if kind == "R":
            frame = f
            call = dev.vvc355_inter_frame_pass
        elif kind == "A":
            frame = abi.AffineFrame(pic=f, cus=d_acu.ptr, jobs_luma=d_ajl.ptr, jobs_chroma=d_ajc.ptr if pic.chroma else 0, n_cus=len(pic.aff), n_jobs=pic.n_aff_jobs)
            call = dev.vvc355_affine_frame_pass
        else:
            frame = abi.GpmFrame(pic=f, cus=d_gcu.ptr, jobs=d_gj.ptr, n_cus=len(pic.gpm), n_jobs=pic.n_gpm_jobs)
            call = dev.vvc355_gpm_frame_pass
        keep += [frame, _up(np.frombuffer(bytes(frame), np.uint8))]
        call(None, pic.bd, keep[-1].ptr, ctypes.addressof(frame))
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    planes = [b.to_host(p.dtype, p.shape)[:, :d[0]].copy() for b, p, d in zip(d_dst, pitched, pic.dims)]
    dmvr = d_dmvr.to_host(np.uint8, (pic.mvf.nbytes,)).view(ifc.MVF_DT).reshape(pic.mvf.shape)
    return planes, dmvr


def _hold(name, want, got, locate):
    bad = sorted(k for k in got if got[k] != want[k])
    if bad:
        pytest.fail(f"{name}: {bad} do not hash to the reference's digests\n" + "\n".join(locate()))


@pytest.mark.parametrize("name", ic.REGULAR + ic.AFFINE + ic.GPM + [ic.MIXED])
def test_stage_drivers_reproduce_the_reference(dev, orc, golden, name):
    pic = ic.picture(name)
    assert ic.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    planes, dmvr = device_picture(dev, pic)
    got = ic.plane_digests(planes)
    if "R" in pic.kinds:
        got["dmvr"] = ic.sha(ic.mvf_bytes(dmvr))
    assert set(got) | {"inputs"} == set(golden[name])

    def locate():
        want = ic.run_picture(orc, "orc", pic)
        lines = ic.plane_differences(pic, want.planes, planes, label="oracle")
        if "R" in pic.kinds:
            lines += ic.dmvr_differences(pic, want.dmvr, dmvr, label="oracle")
        return lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_ref_inter_cpu.py)"]
    _hold(name, golden[name], got, locate)


@pytest.mark.parametrize("name", ic.CIIP)
def test_ciip_driver_reproduces_the_reference(dev, orc, golden, name):
    cp = ic.ciip_picture(name)
    p = cp.p
    assert ic.ciip_inputs_digest(cp) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    run = cc.DeviceRun(dev, p, cp.bd, cp.dims, cp.refs, cp.lut, cp.sentinel)
    err = run.run()
    assert err == 0, f"vvc355_ciip_frame_pass refused the frame: {err}"
    dev.vvc355_stream_sync(None)
    got_run = SimpleNamespace(scratch=run.scratch(), planes=[run.plane(c).copy() for c in range(cp.n_comp)], joint=run.cmds()["joint"])
    got = {**ic.plane_digests(got_run.planes), "scratch": ic.sha(got_run.scratch), "joint": ic.sha(got_run.joint)}
    assert set(got) | {"inputs", "weights"} == set(golden[name])

    def locate():
        want = ic.run_ciip(orc, "orc", cp)
        got_run.weights = want.weights
        lines = ic.ciip_differences(cp, want, got_run, label="oracle")
        exp = ic.ciip_joint(cp, want.weights)
        bad = np.nonzero(exp != got_run.joint)[0]
        if len(bad):
            k = p.cmds[bad[0]]
            lines.append(f"{name}: .joint of command {bad[0]} (component {k['c_idx']} of the unit at ({k['x0']}, {k['y0']})): oracle {exp[bad[0]]}, device {got_run.joint[bad[0]]}")
        return lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_ref_inter_cpu.py)"]
    _hold(name, golden[name], got, locate)

"""GPU: the stage drivers on the full-scale worst-case pictures of tests/extreme_cases.py, held to the reference's digests
(tests/golden/ref_extremes.json), with no oracle in between and no tolerance:

* vvc355_inter_frame_pass (XR*: planes and tab_dmvr_mvf), vvc355_affine_frame_pass (XA*), vvc355_gpm_frame_pass (XG*) and
  vvc355_ciip_frame_pass (XI0: scratch, planes, the patched .joint bytes);
* vvc355_sao_frame_pass (XS*) and vvc355_alf_frame_pass, build + filter (XF*, the CC-ALF pictures XF11-XF14 among them);
* the ALF pictures once more through vvc355_picture_pass's filter half, the path the benchmark takes.
The destination planes start sentinel-filled and are read back whole: the picture has to hash to the digest and the pitch padding has to
hold the sentinel still.  On a mismatch the oracle runs the same picture and the message names the picture, the component, the first
differing sample and both values."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import affine_gpm_cases as agc
import ciip_frame_cases as cc
import extreme_cases as xc
import inter_frame_cases as ifc
import picture_cases as pcs
import ref_inter_cases as ic
import ref_pass_cases as pc
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu
SENTINEL = 0x21


class Device:
    """Uploads that stay alive until the test ends."""

    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        self.keep.append(batch.DeviceBuffer.from_host(a.view(np.uint8) if a.dtype.kind == "V" else a))
        return self.keep[-1]

    def frame(self, f):
        self.keep.append(f)
        return self.up(np.frombuffer(bytes(f), np.uint8)).ptr, ctypes.addressof(f)

    def planes(self, planes):
        pitched = [batch.to_pitched(p) for p in planes]
        return pitched, [self.up(p) for p in pitched]

    def sync(self):
        self.dev.vvc355_stream_sync(None)


@pytest.fixture(scope="module")
def golden():
    return xc.load_golden()


def _whole(name, stage, bufs, pitched, planes):
    """The device planes read back whole: the pictures, after the padding of every row was found to hold the sentinel still."""
    out = []
    for c, (b, p, q) in enumerate(zip(bufs, pitched, planes)):
        got = b.to_host(p.dtype, p.shape)
        bad = np.argwhere(got[:, q.shape[1]:] != SENTINEL)
        assert len(bad) == 0, f"{name} {stage}: component {c}: {len(bad)} samples of the pitch padding were written, first at (row, col) " \
                              f"{[int(bad[0][0]), int(bad[0][1]) + q.shape[1]]}: {got[bad[0][0], bad[0][1] + q.shape[1]]}"
        out.append(got[:, :q.shape[1]].copy())
    return out


def _filter_frame(d, fp, stage):
    """The frame of one stage over freshly uploaded pitched planes -> (frame, alf work address, output buffers, pitched shapes)."""
    t = fp.t
    pitched, bufs = d.planes(fp.planes)
    out_pitched = [np.full_like(p, SENTINEL) for p in pitched]
    out_bufs = [d.up(p) for p in out_pitched]
    tabs = {"sao": d.up(fp.sao), "alf": d.up(fp.alf), "slice_idx": d.up(t.slice_idx), "col_bd": d.up(t.col_bd), "row_bd": d.up(t.row_bd)}
    tabs["slices"] = d.up(np.frombuffer(bytes(pc.alf_slices(fp, [d.up(a).ptr for a in fp.aps])), np.uint8))
    strides = [p.strides[0] for p in pitched]
    f = (pc.sao_frame if stage == "sao" else pc.alf_frame)(fp, [b.ptr for b in out_bufs], [b.ptr for b in bufs], strides, strides, lambda n: tabs[n].ptr)
    work = d.up(np.zeros(d.dev.vvc355_alf_frame_work_bytes(t.cw * t.ch), np.uint8)).ptr if stage == "alf" else 0
    return f, work, out_bufs, out_pitched


def _hold(orc, golden, fp, stage, got):
    rec = pc.stage_digests({stage: got}, (stage,))
    bad = [k for k in rec if rec[k] != golden[fp.name][k]]
    if bad:
        lines = pc.plane_differences(fp.name, stage, pc.run_filter(orc, "orc", fp, stage), got, label="oracle")
        pytest.fail(f"{fp.name}: {bad} do not hash to the reference's digests\n" + "\n".join(
            lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_extremes_cpu.py)"]))


@pytest.mark.parametrize("name", xc.SAO + xc.ALF + xc.ALF_CC)
def test_filter_drivers_reproduce_the_reference(dev, orc, golden, name):
    fp = xc.filter_picture(name)
    assert pc.filter_inputs_digest(fp) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    (stage,) = fp.stages
    d = Device(dev)
    f, work, out_bufs, out_pitched = _filter_frame(d, fp, stage)
    if stage == "sao":
        dev.vvc355_sao_frame_pass(None, fp.bd, *d.frame(f))
    else:
        dev.vvc355_alf_frame_pass(None, fp.bd, *d.frame(f), work)
    d.sync()
    assert dev.vvc355_last_error() == 0
    _hold(orc, golden, fp, stage, _whole(name, stage, out_bufs, out_pitched, fp.planes))


@pytest.mark.parametrize("name", xc.ALF + xc.ALF_CC)
def test_alf_through_the_picture_pass(dev, orc, golden, name):
    """The filter half of vvc355_picture_pass with the ALF stage alone: what the benchmark's chain calls."""
    fp = xc.filter_picture(name)
    d = Device(dev)
    f, work, out_bufs, out_pitched = _filter_frame(d, fp, "alf")
    assert pcs.run(dev, None, fp.bd, pcs.picture({"alf": (d.frame(f)[0], f)}, alf_work=work)) == 0
    d.sync()
    assert dev.vvc355_last_error() == 0
    _hold(orc, golden, fp, "alf", _whole(name, "alf", out_bufs, out_pitched, fp.planes))


# ---------------------------------------------------------------------------------------------------------------- inter pictures

def _device_inter(dev, pic):
    """The picture's units through their stage driver on pitched planes that hold the picture's sentinel everywhere, padding included:
    (whole pitched planes, tab_dmvr_mvf)."""
    d = Device(dev)
    dt = ic.px(pic.bd)
    pitches = [batch.plane_pitch(w, pic.isz) for (w, _h) in pic.dims]
    pitched = [np.full((ph, pitches[c] // pic.isz), pic.sentinel, dt) for c, (_pw, ph) in enumerate(pic.dims[:pic.n_comp])]
    d_dst = [d.up(p) for p in pitched]
    d_ref = [[[d.up(batch.to_pitched(pic.refs[l][r][c])) for c in range(3)] for r in range(2)] for l in range(2)]
    reft = agc.ref_table([[[d_ref[l][r][c].ptr for c in range(3)] for r in range(2)] for l in range(2)], [[pitches] * 2] * 2)
    d_reft, d_mvf, d_dmvr = d.up(np.frombuffer(bytes(reft), np.uint8)), d.up(pic.mvf), d.up(pic.mvf)
    d_sl, d_lut = d.up(np.frombuffer(bytes(pic.slices), np.uint8)), d.up(pic.lut)
    scratch = lambda n: d.up(np.zeros(max(int(n), 64), np.uint8))          # noqa: E731
    d_pus, d_acu, d_gcu = (d.up(a) if len(a) else scratch(0) for a in (pic.pus, pic.aff, pic.gpm))
    d_jl, d_jc, d_rec = scratch(pic.n_jobs * agc.BIPRED_JOB_DT.itemsize), scratch(2 * pic.n_jobs * agc.BIPRED_JOB_DT.itemsize), scratch(pic.n_jobs * 32)
    d_ajl, d_ajc = scratch(pic.n_aff_jobs * agc.AFFINE_JOB_DT.itemsize), scratch(pic.n_aff_chroma_jobs() * agc.BIPRED_JOB_DT.itemsize)
    d_gj = scratch(pic.n_gpm_jobs * agc.GPM_JOB_DT.itemsize)
    f = pic.frame([b.ptr for b in d_dst] + [0] * (3 - pic.n_comp), pitches, d_mvf.ptr, d_reft.ptr, d_sl.ptr, d_lut.ptr, d_pus.ptr, d_jl.ptr, d_jc.ptr,
                  d_rec.ptr, d_dmvr.ptr)
    if pic.kinds == "R":
        frame, call = f, dev.vvc355_inter_frame_pass
    elif pic.kinds == "A":
        frame = abi.AffineFrame(pic=f, cus=d_acu.ptr, jobs_luma=d_ajl.ptr, jobs_chroma=d_ajc.ptr if pic.chroma else 0, n_cus=len(pic.aff), n_jobs=pic.n_aff_jobs)
        call = dev.vvc355_affine_frame_pass
    else:
        frame = abi.GpmFrame(pic=f, cus=d_gcu.ptr, jobs=d_gj.ptr, n_cus=len(pic.gpm), n_jobs=pic.n_gpm_jobs)
        call = dev.vvc355_gpm_frame_pass
    call(None, pic.bd, *d.frame(frame))
    d.sync()
    assert dev.vvc355_last_error() == 0
    whole = [b.to_host(p.dtype, p.shape) for b, p in zip(d_dst, pitched)]
    dmvr = d_dmvr.to_host(np.uint8, (pic.mvf.nbytes,)).view(ifc.MVF_DT).reshape(pic.mvf.shape)
    return whole, dmvr


@pytest.mark.parametrize("name", xc.REGULAR + xc.AFFINE + xc.GPM)
def test_inter_drivers_reproduce_the_reference(dev, orc, golden, name):
    pic, _ = xc.inter_picture(name)
    assert ic.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    whole, dmvr = _device_inter(dev, pic)
    planes = []
    for c, (p, (w, _h)) in enumerate(zip(whole, pic.dims)):
        bad = np.argwhere(p[:, w:] != pic.sentinel)
        assert len(bad) == 0, f"{name}: component {c}: {len(bad)} samples of the pitch padding were written, first at (row, col) {[int(bad[0][0]), int(bad[0][1]) + w]}"
        planes.append(p[:, :w].copy())
    got = ic.plane_digests(planes)
    if "R" in pic.kinds:
        got["dmvr"] = ic.sha(ic.mvf_bytes(dmvr))
    assert set(got) | {"inputs"} == set(golden[name])
    bad = sorted(k for k in got if got[k] != golden[name][k])
    if bad:
        want = ic.run_picture(orc, "orc", pic)
        lines = ic.plane_differences(pic, want.planes, planes, label="oracle")
        if "R" in pic.kinds:
            lines += ic.dmvr_differences(pic, want.dmvr, dmvr, label="oracle")
        pytest.fail(f"{name}: {bad} do not hash to the reference's digests\n" + "\n".join(
            lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_extremes_cpu.py)"]))


def test_ciip_driver_reproduces_the_reference(dev, orc, golden):
    """XI0 through vvc355_ciip_frame_pass: the scratch whole, the planes and the .joint bytes of the patched commands."""
    name = "XI0"
    cp, _ = xc.ciip_picture(name)
    p = cp.p
    assert ic.ciip_inputs_digest(cp) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    run = cc.DeviceRun(dev, p, cp.bd, cp.dims, cp.refs, cp.lut, cp.sentinel)
    err = run.run()
    assert err == 0, f"vvc355_ciip_frame_pass refused the frame: {err}"
    dev.vvc355_stream_sync(None)
    assert dev.vvc355_last_error() == 0
    got_run = SimpleNamespace(scratch=run.scratch(), planes=[run.plane(c).copy() for c in range(cp.n_comp)], joint=run.cmds()["joint"])
    got = {**ic.plane_digests(got_run.planes), "scratch": ic.sha(got_run.scratch), "joint": ic.sha(got_run.joint)}
    assert set(got) | {"inputs", "weights"} == set(golden[name])
    bad = sorted(k for k in got if got[k] != golden[name][k])
    if bad:
        want = ic.run_ciip(orc, "orc", cp)
        got_run.weights = want.weights
        lines = ic.ciip_differences(cp, want, got_run, label="oracle")
        exp = ic.ciip_joint(cp, want.weights)
        first = np.nonzero(exp != got_run.joint)[0]
        if len(first):
            k = p.cmds[first[0]]
            lines.append(f"{name}: .joint of command {first[0]} (component {k['c_idx']} of the unit at ({k['x0']}, {k['y0']})): oracle {exp[first[0]]}, device {got_run.joint[first[0]]}")
        pytest.fail(f"{name}: {bad} do not hash to the reference's digests\n" + "\n".join(
            lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_extremes_cpu.py)"]))

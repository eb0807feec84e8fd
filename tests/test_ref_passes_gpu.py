"""GPU: the in-loop filter stage drivers held to the reference's own digests (tests/golden/ref_passes.json: what ff_vvc_deblock_vertical /
_horizontal, ff_vvc_sao_filter and ff_vvc_alf_filter computed on the pictures of tests/ref_pass_cases.py), with no oracle in between:

* vvc355_deblock_bs_pass: the ten bS / filter-length tables;
* vvc355_deblock_frame_pass, vertical then horizontal, on pitched planes: every plane after either pass;
* the record path for every picture with minimum coding block 4: vvc355_tab_fill_pass (motion only), vvc355_deblock_bs_rec_pass,
  vvc355_deblock_qp_rec_pass, then the two frame passes, to the same digests;
* vvc355_sao_frame_pass and vvc355_alf_frame_pass;
* C0 chained on device-resident tables, after every stage.
The 4:0:0 pictures pass n_comp = 1.  Only the committed digests are read.  On a mismatch the oracle runs the same picture (it reproduces the
same digests, tests/test_ref_passes_cpu.py) and the message names the first differing unit or sample."""
import ctypes

import numpy as np
import pytest

import bs_rec_cases as rc
import qp_rec_cases as qc
import ref_pass_cases as pc
from ffvvc_amd import batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


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


def _download(bufs, pitched, planes):
    return [b.to_host(p.dtype, p.shape)[:, :q.shape[1]].copy() for b, p, q in zip(bufs, pitched, planes)]


def _output_tables(d, pic):
    """Device output tables: 0xEE where the pass has to write every entry, zero where (4:0:0) it writes none, like the other sides."""
    t = pic.t
    return {n: d.up(np.full((t.th, t.tw), 0xEE if pic.n_comp == 3 or n in ("bs00", "bs10", "p0", "p1", "q0", "q1") else 0, np.uint8)) for n in t.OUT}


def _frame_passes(d, pic, planes, addr, out):
    pitched, bufs = d.planes(planes)
    for vertical in (1, 0):
        f = pc.deblock_frame(pic, vertical, [b.ptr for b in bufs], [p.strides[0] for p in pitched], addr)
        d.dev.vvc355_deblock_frame_pass(None, pic.bd, *d.frame(f))
        d.sync()
        out["v" if vertical else "h"] = _download(bufs, pitched, planes)
    return bufs, pitched


def device_deblock(dev, pic, planes=None):
    """vvc355_deblock_bs_pass on the picture's tables, then both frame passes: the same dict as ref_pass_cases.run_deblock, plus the device
    handles under "_dev" (tables, plane buffers, pitched shapes) for a caller that goes on."""
    d, t = Device(dev), pic.t
    tabs = {n: d.up(a) for n, a in pic.arrays.items()}
    tabs.update(_output_tables(d, pic))
    addr = lambda n: tabs[n].ptr          # noqa: E731
    dev.vvc355_deblock_bs_pass(None, *d.frame(pc.bs_frame(pic, addr)))
    d.sync()
    out = {n: tabs[n].to_host(np.uint8, (t.th, t.tw)) for n in t.OUT}
    src = planes if planes is not None else pic.planes
    bufs, pitched = _frame_passes(d, pic, src, addr, out)
    out["_dev"] = (d, tabs, bufs, pitched)
    return out


def device_deblock_records(dev, pic):
    """The record path: MvField table from the motion records, boundary strengths and QP tables from the unit records, then both frame passes."""
    d, t, p = Device(dev), pic.t, pic.rec
    (cu, cu_first), (tu, tu_first), (mv, mv_first) = rc.grouped(t)
    assert np.array_equal(cu, p.cu) and np.array_equal(tu, p.tu)
    chroma = pic.n_comp == 3
    tabs = _output_tables(d, pic)
    for n in rc.TB_C + qc.TABLES:
        tabs[n] = d.up(np.full((t.th, t.tw), 0xEE, np.uint8))
    tabs["mvf"] = batch.DeviceBuffer(t.mvf.nbytes)
    for n in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
        tabs[n] = d.up(getattr(t, n))
    tabs["dbp"] = d.up(pic.arrays["dbp"])
    addr = lambda n: tabs[n].ptr          # noqa: E731
    d_cu, d_cu_first, d_tu, d_tu_first, d_cu_qp, d_tu_qp_c = (d.up(a) for a in (cu, cu_first, tu, tu_first, p.cu_qp, p.tu_qp_c))
    rc.fill_mvf(dev, t, mv, mv_first, tabs["mvf"], None, d.keep)
    cu_arg, tu_arg = (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr)
    bf = rc.rec_frame(t, cu_arg, tu_arg, addr, pic.n_comp, tb_c=chroma)
    err = dev.vvc355_deblock_bs_rec_pass(None, *d.frame(bf))
    assert err == 0, f"vvc355_deblock_bs_rec_pass refused the frame: {err}"
    qf = qc.qp_frame(t, cu_arg, tu_arg if chroma else (0, 0, 0), d_cu_qp.ptr, d_tu_qp_c.ptr if chroma else 0,
                     [tabs[n].ptr if chroma or n == "qp_y" else 0 for n in qc.TABLES], t.tw, pic.n_comp)
    err = dev.vvc355_deblock_qp_rec_pass(None, *d.frame(qf))
    assert err == 0, f"vvc355_deblock_qp_rec_pass refused the frame: {err}"
    d.sync()
    out = {n: tabs[n].to_host(np.uint8, (t.th, t.tw)) for n in t.OUT}
    for n in qc.TABLES[:pic.n_comp]:
        got = tabs[n].to_host(np.int8, (t.th, t.tw))
        bad = np.argwhere(got != pic.arrays[n])
        assert len(bad) == 0, f"{pic.name}: {n} from the records differs from the painted table in {len(bad)} units, first at {bad[0].tolist()}"
    _frame_passes(d, pic, pic.planes, addr, out)
    return out


def device_filter(dev, fp, stage, planes=None, src_bufs=None):
    """vvc355_sao_frame_pass / vvc355_alf_frame_pass of `planes` (or of the device planes `src_bufs` = (buffers, pitched shapes)) into planes
    pre-filled with 0x21.  Returns (filtered planes, (buffers, pitched shapes), the Device that keeps them)."""
    d, t = Device(dev), fp.t
    like = planes if planes is not None else fp.planes
    bufs, pitched = src_bufs if src_bufs is not None else d.planes(like)[::-1]
    out_pitched = [np.full_like(p, 0x21) for p in pitched]
    out_bufs = [d.up(p) for p in out_pitched]
    tabs = {"sao": d.up(fp.sao), "alf": d.up(fp.alf), "slice_idx": d.up(t.slice_idx), "col_bd": d.up(t.col_bd), "row_bd": d.up(t.row_bd)}
    tabs["slices"] = d.up(np.frombuffer(bytes(pc.alf_slices(fp, [d.up(a).ptr for a in fp.aps])), np.uint8))
    make = pc.sao_frame if stage == "sao" else pc.alf_frame
    strides = [p.strides[0] for p in pitched]
    f = make(fp, [b.ptr for b in out_bufs], [b.ptr for b in bufs], strides, strides, lambda n: tabs[n].ptr)
    if stage == "sao":
        dev.vvc355_sao_frame_pass(None, fp.bd, *d.frame(f))
    else:
        work = d.up(np.zeros(dev.vvc355_alf_frame_work_bytes(t.cw * t.ch), np.uint8))
        dev.vvc355_alf_frame_pass(None, fp.bd, *d.frame(f), work.ptr)
    d.sync()
    return _download(out_bufs, out_pitched, like), (out_bufs, out_pitched), d


def _hold(name, want_rec, got, stages, tables, locate):
    rec = pc.stage_digests(got, stages, tables)
    bad = [k for k in rec if rec[k] != want_rec[k]]
    if bad:
        pytest.fail(f"{name}: {bad} do not hash to the reference's digests\n" + "\n".join(locate()))


def _locate_deblock(orc, pic, got, planes=None):
    want = pc.run_deblock(orc, "orc", pic, planes)
    lines = pc.table_differences(pic, want, got, label="oracle")
    for s in ("v", "h"):
        lines += pc.plane_differences(pic.name, s, want[s], got[s], label="oracle")
    return lines or ["the oracle agrees with the device: the oracle no longer reproduces the digests either (tests/test_ref_passes_cpu.py)"]


@pytest.mark.parametrize("name", pc.DEBLOCK)
def test_deblocking_from_tables(dev, orc, golden, name):
    pic = pc.deblock_picture(orc, name)
    assert pc.deblock_inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    got = device_deblock(dev, pic)
    _hold(name, golden[name], got, ("v", "h"), pic.t.OUT, lambda: _locate_deblock(orc, pic, got))


@pytest.mark.parametrize("name", pc.REC_PATH)
def test_deblocking_from_records(dev, orc, golden, name):
    pic = pc.deblock_picture(orc, name)
    got = device_deblock_records(dev, pic)
    _hold(name, golden[name], got, ("v", "h"), pic.t.OUT, lambda: _locate_deblock(orc, pic, got))


@pytest.mark.parametrize("name", pc.FILTER)
def test_sao_and_alf(dev, orc, golden, name):
    fp = pc.filter_picture(name)
    assert pc.filter_inputs_digest(fp) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    got = {s: device_filter(dev, fp, s)[0] for s in ("sao", "alf")}
    _hold(name, golden[name], got, ("sao", "alf"), (),
          lambda: sum((pc.plane_differences(name, s, pc.run_filter(orc, "orc", fp, s), got[s], label="oracle") for s in ("sao", "alf")), []))


def test_chain_on_device_resident_tables(dev, orc, golden):
    """C0: bS, vertical, horizontal, SAO, ALF, each stage on what the previous one left in device memory."""
    d, fp = pc.chain_picture()
    got = device_deblock(dev, d)
    _dev, _tabs, bufs, pitched = got.pop("_dev")
    got["sao"], sao_bufs, keep_sao = device_filter(dev, fp, "sao", d.planes, (bufs, pitched))
    got["alf"], _, keep_alf = device_filter(dev, fp, "alf", d.planes, sao_bufs)

    def locate():
        want = pc.run_chain(orc, "orc")
        lines = pc.table_differences(d, want, got, label="oracle")
        for s in ("v", "h", "sao", "alf"):
            lines += pc.plane_differences(pc.CHAIN, s, want[s], got[s], label="oracle")
        return lines
    _hold(pc.CHAIN, golden[pc.CHAIN], got, ("v", "h", "sao", "alf"), d.t.OUT, locate)

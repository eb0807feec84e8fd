"""The directed worst-case pictures of tests/recon_extreme_cases.py on the device, held to the reference's digests
(tests/golden/ref_recon_extremes.json): HIP == ff_vvc_reconstruct on planes of 0 and the maximum, sign-matched levels at and beyond the
ends of int16, the LMCS model with the smallest and largest codeword counts.  Reads the committed digests and oracle/liborc.so only.

Every listed picture is recorded (vvc355_rec_*, packing on) and the recorder's arrays — commands bound to the device arena, CTU table, ticket
order, the three record lists with their side records, the packed level stream, the arena — are uploaded as they are, after they were
compared with the inputs derived by INTEGRATION.md's rules (recorder_cases.differences); the runs with int32 levels upload the derived
inputs as tests/test_ref_recon_gpu.py does (its DevicePicture).  Every picture runs
  * through the separate entries — vvc355_intra_tb_pass, vvc355_inter_tb_pass / vvc355_ts_tb_pass around vvc355_lmcs_vpdu_scale_pass,
    vvc355_recon_frame_pass, then vvc355_lmcs_frame_pass — in vvc355_recon_order's ticket order, two pictures in raster order as well;
  * through ONE vvc355_picture_pass with the filter half off (the same stages, inverse LMCS included);
  * with the packed int16 level stream; two pictures also with int32 levels in place;
  * twice on the same state buffers and command array (planes, arena and scale table uploaded afresh), as the walk tests do;
  * and, where the older job path can express it (recon_extreme_cases.OLD_PATH), through vvc355_itx_frame_build, the shape batches and
    vvc355_lmcs_chroma_resid_batch.
Planes carry sentinel bytes in the pitch padding and sentinel rows above and below, and are read back whole.  The reconstruction is compared
with the digests; inverse LMCS (a table look-up under the slices' flags) with numpy on the reconstruction the digests hold.  A failure names
the first differing sample against the oracle side, which tests/test_recon_extremes_cpu.py holds to the same digests.

Nothing unchecked reaches the device: ref_recon_cases.well_formed and vvc355_recon_order_check run on every list before its launch."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import inter_tb_cases as tc
import levels_cases as lc
import picture_cases as pcs
import recon_cases
import recon_extreme_cases as xc
import recorder_cases as rk
import recorder_chain_cases as ch
import ref_recon_cases as rc
import test_ref_recon_gpu as base
from ffvvc_amd import abi

pytestmark = pytest.mark.gpu

GUARD = 2                                   # sentinel rows above and below every plane
# (picture, levels, ticket order)
RUNS = ([(n, "packed", "critical") for n in xc.picture_names()] + [(n, "packed", "raster") for n in xc.RASTER_TOO] +
        [(n, "int32", "critical") for n in xc.UNPACKED_TOO])


@pytest.fixture(scope="module")
def golden():
    return xc.load_golden()


_oracle = {}


def oracle_planes(name):
    """The oracle side's reconstruction of a picture (for the inverse-LMCS expectation and for naming a first difference)."""
    if name not in _oracle:
        import ref_lib
        _oracle[name] = rc.oracle_side(ref_lib.load_oracle(), rc.derive(xc.picture(name)))[0]
    return _oracle[name]


def _checked(dev, name, order_kind):
    pic = xc.picture(name)
    d = rc.derive(pic)
    bad = rc.well_formed(pic, d)
    assert bad is None, f"{name}: {bad}: not launched"
    order = recon_cases.critical_order(dev, d.ctus, pic.ncx, pic.ncy) if order_kind == "critical" else d.order
    assert rc.order_defect(d.ctus, pic.ncx, pic.ncy, order) is None, f"{name}: not launched"
    assert pcs.order_check(dev, d.ctus, pic.ncx, pic.ncy, order) == 0, f"{name}: vvc355_recon_order_check refuses the {order_kind} order: not launched"
    return pic, d, np.ascontiguousarray(order, np.int32)


class Recorded(base.DevicePicture):
    """The picture through the recorder with packing on, the snapshot's arrays uploaded as they are; the runs and the read-back are
    test_ref_recon_gpu.DevicePicture's.  order: a ticket order to use in place of the recorder's."""

    def __init__(self, dev, pic, d, k, host, planes, order=None):
        self.dev, self.pic, self.d, self.k = dev, pic, d, k
        rec = dev.vvc355_rec_create()
        try:
            o = self.o = rk.record(dev, pic, True, rec=rec)
            bad = rk.differences(dev, pic, d, o, True)
            assert not bad, f"{pic.name}: the recorder's {bad} differ from the derived inputs: not launched"
            self.arena0 = o.arena if o.arena_len else np.zeros(4, np.int32)
            self.d_arena = k.up(self.arena0)
            assert dev.vvc355_rec_bind(rec, self.d_arena.ptr) == 0
            cmds = rk._copy(o.res.cmds, o.res.n_cmds, rk.CMD)
        finally:
            dev.vvc355_rec_destroy(rec)
        wide = (o.lv["flags"] & abi.LEVELS_INT32) != 0
        assert wide.any() and not wide.all() and (o.levels == 32767).any() and (o.levels == -32768).any()
        self.order = o.order if order is None else order
        assert pcs.order_check(dev, o.ctus, pic.ncx, pic.ncy, self.order) == 0 and rc.order_defect(o.ctus, pic.ncx, pic.ncy, self.order) is None, "not launched"
        self.host_planes, self.d_planes = host, planes
        strides = [p.shape[1] * pic.isz for p in host]
        self.stages, self.scaled, self.d_table, _cmds, _maps = ch.recorded_stages(k, dev, pic, d, o, cmds, self.d_arena, planes, strides, self.order)
        self.table0 = np.full(d.tpic.ux * d.tpic.uy, -1, np.int16)


class Guarded:
    """The picture on the device over planes with sentinel rows around them, plus the inverse-LMCS stage: Recorded for packed levels,
    test_ref_recon_gpu.DevicePicture on the derived inputs for int32 levels.  restart() puts planes, arena and scale table back and leaves
    the state buffers and the command array as the last run left them."""

    def __init__(self, dev, pic, d, levels, order, order_kind="critical"):
        k = self.k = pcs.Keep()
        host = [tc.pitched(p) for p in pic.planes]
        self.planes = [ch.GuardedPlane(k, p, GUARD) for p in host]
        if levels == "packed":
            dp = self.dp = Recorded(dev, pic, d, k, host, self.planes, order if order_kind == "raster" else None)
        else:
            holder = SimpleNamespace(host=host, d_planes=self.planes, d_table=k.up(np.full(d.tpic.ux * d.tpic.uy, -1, np.int16)))
            dp = self.dp = base.DevicePicture(dev, pic, d, levels, order, shared=(k.up(rc.start_arena(d, None)), holder))
        self.used = np.array([sl[1] for sl in pic.slices], np.uint8)
        self.lut = xc.inverse_lut(pic)
        shape = SimpleNamespace(width=pic.width, height=pic.height, cw=pic.ncx, ch=pic.ncy, n_slices=len(pic.slices), ctb_log2=pic.ctb_log2,
                                pitch=host[0].shape[1] * pic.isz)
        dp.stages["lmcs"] = k.frame(pcs.lmcs_frame(shape, self.planes[0].ptr, k.up(self.lut).ptr, k.up(pic.slice_idx).ptr, k.up(self.used).ptr))
        self.dev, self.pic = dev, pic

    def restart(self):
        dp, up = self.dp, self.dev.vvc355_upload
        for p in self.planes:
            up(p.buf.ptr, p.full.ctypes.data, p.full.nbytes)
        up(dp.d_arena.ptr, dp.arena0.ctypes.data, dp.arena0.nbytes)
        up(dp.d_table.ptr, dp.table0.ctypes.data, dp.table0.nbytes)

    def inverse_lmcs(self):
        st = self.dp.stages["lmcs"]
        assert self.dev.vvc355_lmcs_frame_pass(None, self.pic.bd, st[0], ctypes.addressof(st[1])) == 0

    def expected_final_luma(self, recon_luma):
        mask = pcs.lmcs_mask(self.pic.width, self.pic.height, self.pic.ctb_log2, self.pic.slice_idx, self.used)
        return np.where(mask, self.lut[recon_luma], recon_luma).astype(recon_luma.dtype)


def _held(name, how, golden, d, planes, table, keys=None):
    got = rc.digests(d.pic, d, planes, table)
    assert set(got) == set(golden[name])
    bad = sorted(k for k in (keys or got) if k != "inputs" and got[k] != golden[name][k])
    why = rc.first_difference(oracle_planes(name), planes) or "the oracle side differs from the digests as well: run tests/test_recon_extremes_cpu.py"
    assert not bad, f"{name} ({how}): {bad} do not hash to the reference's digests: {why}"


@pytest.mark.parametrize("name,levels,order_kind", RUNS)
def test_separate_entries_reproduce_the_reference_digests(dev, golden, name, levels, order_kind):
    pic, d, order = _checked(dev, name, order_kind)
    assert rc.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    g = Guarded(dev, pic, d, levels, order, order_kind)
    for rep in range(2):
        how = f"entries, {levels} levels, {order_kind} order, pass {rep}"
        g.restart()
        g.dp.run_entries()
        planes, table = g.dp.result()
        _held(name, how, golden, d, planes, table)
        g.inverse_lmcs()
        final, _table = g.dp.result()
        want = g.expected_final_luma(planes[0])
        assert np.array_equal(final[0], want), f"{name} ({how}): inverse LMCS: {rc.first_difference([want], [final[0]])}"
        assert all(np.array_equal(a, b) for a, b in zip(planes[1:], final[1:])), f"{name} ({how}): inverse LMCS wrote chroma"
        assert bool(g.used.any()) == (not np.array_equal(final[0], planes[0])), f"{name}: inverse LMCS changes luma exactly where a slice uses it"


@pytest.mark.parametrize("name", xc.picture_names())
def test_one_picture_pass_reproduces_the_reference_digests(dev, golden, name):
    pic, d, order = _checked(dev, name, "critical")
    assert rc.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    g = Guarded(dev, pic, d, "packed", order)
    recon = oracle_planes(name)
    assert rc.sha(recon[0]) == golden[name]["p0"], "the oracle side differs from the digests: run tests/test_recon_extremes_cpu.py"
    inside = recon[0][pcs.lmcs_mask(pic.width, pic.height, pic.ctb_log2, pic.slice_idx, g.used)]
    assert not g.used.any() or ((inside == 0).any() and (inside == (1 << pic.bd) - 1).any()), "luma inside the LMCS slices misses an end of the range"
    assert set(g.dp.stages) <= {"intra_tb", "inter_tb", "ts_tb", "lmcs_scale", "recon", "lmcs"} and ("lmcs_scale" in g.dp.stages) == bool(pic.chroma_scale_flag)
    want = g.expected_final_luma(recon[0])
    for rep in range(2):
        how = f"one picture pass, pass {rep}"
        g.restart()
        g.dp.run_picture()
        planes, table = g.dp.result()
        assert np.array_equal(planes[0], want), f"{name} ({how}): luma after inverse LMCS: {rc.first_difference([want], [planes[0]])}"
        _held(name, how, golden, d, [recon[0]] + planes[1:], table)


@pytest.mark.parametrize("name", xc.OLD_PATH)
def test_older_job_path_reproduces_the_reference_digests(dev, orc, golden, name):
    """The path the inter record pass replaced, for the transformed blocks of the inter units (inter_tb_cases.OldPath), the other stages as
    before: test_ref_recon_gpu.py's run on the worst-case content."""
    tc.bind_oracle(orc)
    pic, d, order = _checked(dev, name, "raster")
    assert len(pic.slices) == 1 and len(set(pic.col_bd[:-1].tolist())) == 1 and d.inter and not any(s["joint"] & 1 for s in d.inter)
    assert all(d.tpic.unit_of(s, "cu") == d.tpic.unit_of(s, "block") for s in d.inter), "the older path takes the unit from the block's position"
    n_i, n_e = len(d.intra), len(d.inter)
    tcd = tc.DevicePicture(d.tpic)
    old = tc.OldPath(orc, d.tpic, d.inter, d.offs[n_i:n_i + n_e], rc.start_arena(d), pic.rbits, None, dpic=tcd)
    dp = base.DevicePicture(dev, pic, d, "int32", order, shared=(old.d_arena, tcd))
    st, bd = dp.stages, pic.bd
    call = lambda nm, fn, *a: fn(None, st[nm][0], ctypes.addressof(st[nm][1]), *a) if nm in st else 0      # noqa: E731
    assert call("intra_tb", dev.vvc355_intra_tb_pass) == 0
    old.build(dev)
    old.shapes(dev)
    if dp.scaled:
        assert sum(1 for s in d.inter if s["joint"] & 8 and not s["keep"]) > 5
        assert call("ts_tb", dev.vvc355_ts_tb_pass, 1) == 0
        tcd.scale_pass(dev)
        old.resid(dev)
        assert call("ts_tb", dev.vvc355_ts_tb_pass, 2) == 0
    else:
        assert call("ts_tb", dev.vvc355_ts_tb_pass, 3) == 0
    dev.vvc355_recon_frame_pass(None, bd, st["recon"][0], ctypes.addressof(st["recon"][1]))
    planes, table = dp.result()
    _held(name, "older job path", golden, d, planes, table)

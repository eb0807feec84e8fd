"""The recorder's output on the device, held to the reference's digests (tests/golden/ref_recon.json): parsed units -> vvc355_rec_* ->
the TB record passes and the RECON walk == ff_vvc_reconstruct, with no numpy derivation in between.  Needs neither the reference library
nor the reference tree.

Every listed picture of tests/ref_recon_cases.py is recorded with packing on; the recorder's arrays are uploaded as they are (the arena
after vvc355_rec_fill_arena, the commands after vvc355_rec_bind on the device arena) and run through the separate entries in
INTEGRATION.md's order — vvc355_intra_tb_pass, vvc355_inter_tb_pass(1), vvc355_ts_tb_pass(1), vvc355_lmcs_vpdu_scale_pass,
vvc355_inter_tb_pass(2), vvc355_ts_tb_pass(2), vvc355_recon_frame_pass; without chroma residual scaling one call of each TB pass with
channels 3.  Two pictures run again with packing off (int32 levels in the arena, no side records), one through ONE vvc355_picture_pass
with the descriptors filled from the vvc355_rec_result.

Before any launch the recorder's output is compared with ref_recon_cases.derive() (recorder_cases.differences, what
tests/test_recorder_cpu.py asserts) and the ticket order is checked by vvc355_recon_order_check: a malformed order makes the walk wait
forever, so nothing unchecked reaches the device."""
import ctypes

import numpy as np
import pytest

import inter_tb_cases as tc
import picture_cases as pcs
import recorder_cases as rk
import ref_recon_cases as rc
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

RUNS = [(name, True, "entries") for name in rc.picture_names()] + [("T2", False, "entries"), ("T5", False, "entries"), ("T5", True, "picture")]


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


_derived = {}


def _listed(name):
    if name not in _derived:
        pic = rc.picture(name)
        _derived[name] = (pic, rc.derive(pic))
    return _derived[name]


class Recorded:
    """One picture recorded and uploaded: planes (pitched), arena, the recorder's three lists, side records and stream, commands bound to
    the device arena, CTU table and order; the frames of the stages filled from the result."""

    def __init__(self, dev, pic, d, pack):
        k = self.k = pcs.Keep()
        self.dev, self.pic = dev, pic
        rec = dev.vvc355_rec_create()
        try:
            o = self.o = rk.record(dev, pic, pack, rec=rec)
            bad = rk.differences(dev, pic, d, o, pack)
            assert not bad, f"{pic.name}: {bad} differ from derive(): not launched"
            assert pcs.order_check(dev, o.ctus, pic.ncx, pic.ncy, o.order) == 0 and rc.order_defect(o.ctus, pic.ncx, pic.ncy, o.order) is None, "not launched"
            self.d_arena = k.up(o.arena if o.arena_len else np.zeros(4, np.int32))
            assert dev.vvc355_rec_bind(rec, self.d_arena.ptr) == 0
            cmds = rk._copy(o.res.cmds, o.res.n_cmds, rk.CMD)
        finally:
            dev.vvc355_rec_destroy(rec)
        is_res = cmds["kind"] == abi.RECON_RESID
        assert np.all((cmds["resid"][is_res] >= self.d_arena.ptr) & (cmds["resid"][is_res] < self.d_arena.ptr + 4 * max(o.arena_len, 1)))
        res, bd = o.res, pic.bd
        self.host_planes = [tc.pitched(p) for p in pic.planes]
        self.d_planes = [k.up(p) for p in self.host_planes]
        strides = [p.shape[1] * pic.isz for p in self.host_planes]
        d_slice, d_col, d_row = (k.up(a) for a in (pic.slice_idx, pic.col_bd, pic.row_bd))
        d_model = k.up(np.frombuffer(bytes(pic.model), np.uint8))
        d_levels = k.up(o.levels) if pack else None
        if d_levels is not None:
            assert d_levels.ptr % 32 == 0
        n_i, n_e, n_s = res.n_intra, res.n_inter, res.n_ts

        def side(first, n):
            return k.up(o.lv[first:first + n].view(np.uint8) if n else np.zeros(16, np.uint8)).ptr if pack else 0

        self.scaled = bool(pic.chroma_scale_flag)
        ux, uy = d.tpic.ux, d.tpic.uy
        self.table0 = np.full(ux * uy, -1, np.int16)
        self.d_table = k.up(self.table0)
        st = {}
        if n_i:
            f = abi.IntraTbFrame()
            f.tus, f.coeffs, f.n_tus = k.up(o.intra).ptr, self.d_arena.ptr, n_i
            for c in range(6):
                f.class_first[c] = res.class_first[c]
            f.range, f.bd = pic.rbits, bd
            f.lv, f.levels = side(0, n_i), d_levels.ptr if pack else 0
            st["intra_tb"] = k.frame(f)
        for name, ty, recs, n, first, first_lv in (("inter_tb", abi.InterTbFrame, o.inter, n_e, res.bin_first, n_i),
                                                   ("ts_tb", abi.TsTbFrame, o.ts, n_s, res.ts_first, n_i + n_e)):
            if not n:
                continue
            f = ty()
            f.tus, f.coeffs, f.n_tus = k.up(recs).ptr, self.d_arena.ptr, n
            for c in range(3):
                f.plane[c], f.stride[c] = self.d_planes[c].ptr, strides[c]
            f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = pic.width, pic.height, pic.hs, pic.vs, pic.size_y, pic.rbits, bd
            f.scale_table = self.d_table.ptr if self.scaled else 0
            dst = f.bin_first if name == "inter_tb" else f.class_first
            for ch in range(2):
                for b in range(len(first[ch])):
                    dst[ch][b] = first[ch][b]
            f.lv, f.levels = side(first_lv, n), d_levels.ptr if pack else 0
            st[name] = k.frame(f)
        if self.scaled:
            st["lmcs_scale"] = k.frame(rc.scale_frame(pic, self.d_planes[0].ptr, strides[0], self.d_table.ptr, d_model.ptr, d_slice.ptr, d_col.ptr, d_row.ptr))
        d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(pic.ncx * pic.ncy))
        k.keep.append(d_state)
        st["recon"] = k.frame(rc.recon_frame(pic, None,[b.ptr for b in self.d_planes], strides, k.up(cmds if len(cmds) else np.zeros(1, rk.CMD)).ptr,
                                             k.up(o.ctus).ptr, k.up(o.order if len(o.order) else np.zeros(1, np.int32)).ptr, d_state.ptr,
                                             d_slice.ptr, d_col.ptr, d_row.ptr, d_model.ptr if self.scaled else 0, n_work=res.n_work))
        self.stages = st

    def run_entries(self):
        dev, st, bd = self.dev, self.stages, self.pic.bd
        call = lambda name, fn, *a: fn(None, st[name][0], ctypes.addressof(st[name][1]), *a) if name in st else 0      # noqa: E731
        assert call("intra_tb", dev.vvc355_intra_tb_pass) == 0
        if self.scaled:
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 1) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 1) == 0
            dev.vvc355_lmcs_vpdu_scale_pass(None, bd, st["lmcs_scale"][0], ctypes.addressof(st["lmcs_scale"][1]))
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 2) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 2) == 0
        else:
            assert call("inter_tb", dev.vvc355_inter_tb_pass, 3) == 0
            assert call("ts_tb", dev.vvc355_ts_tb_pass, 3) == 0
        dev.vvc355_recon_frame_pass(None, bd, st["recon"][0], ctypes.addressof(st["recon"][1]))

    def run_picture(self):
        ret = pcs.run(self.dev, None, self.pic.bd, pcs.picture(self.stages, recon_tables=(self.o.ctus, self.o.order)))
        assert ret == 0, f"vvc355_picture_pass refused the picture: stage / code {pcs.decode(ret)}"

    def result(self):
        self.dev.vvc355_stream_sync(None)
        assert self.dev.vvc355_last_error() == 0
        planes = [b.to_host(h.dtype, h.shape) for b, h in zip(self.d_planes, self.host_planes)]
        for c, (g, h, p) in enumerate(zip(planes, self.host_planes, self.pic.planes)):
            assert np.array_equal(g[:, p.shape[1]:], h[:, p.shape[1]:]), f"component {c}: the pitch padding was written"
        table = self.d_table.to_host(np.int16, self.table0.shape) if self.scaled else None
        return [g[:, :p.shape[1]] for g, p in zip(planes, self.pic.planes)], table


@pytest.mark.parametrize("name,pack,how", RUNS)
def test_recorded_pictures_reproduce_the_reference_digests(dev, golden, name, pack, how):
    pic, d = _listed(name)
    assert rc.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    r = Recorded(dev, pic, d, pack)
    (r.run_entries if how == "entries" else r.run_picture)()
    planes, table = r.result()
    got = rc.digests(pic, d, planes, table)               # d gives the units whose scale is compared: the recorder's batched blocks are derive()'s
    assert set(got) == set(golden[name])
    bad = sorted(k for k in got if k != "inputs" and got[k] != golden[name][k])
    assert not bad, f"{name} ({how}, packing {'on' if pack else 'off'}): {bad} do not hash to the reference's digests"

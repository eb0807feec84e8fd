"""The RECON walk and the TB record passes on the device, held to the reference's digests (tests/golden/ref_recon.json): HIP ≡ ff_vvc_reconstruct
with no oracle in between.  Needs neither the reference library nor the reference tree.

Every listed picture of tests/ref_recon_cases.py runs from the inputs derived by INTEGRATION.md's rules
  * through the separate entries in its order — vvc355_intra_tb_pass, vvc355_inter_tb_pass(1), vvc355_ts_tb_pass(1),
    vvc355_lmcs_vpdu_scale_pass, vvc355_inter_tb_pass(2), vvc355_ts_tb_pass(2), vvc355_recon_frame_pass (without chroma residual scaling: one
    call of the two passes with both channel types) — and through ONE vvc355_picture_pass;
  * with int32 levels in place in the arena, and with the packed int16 stream;
  * with ascending raster ticket order and with vvc355_recon_order's;
  * and, on the two pictures it can express (ref_recon_cases.OLD_PATH), through the older job path that inter_tb_cases already drives:
    vvc355_itx_frame_build and the shape batches, then vvc355_lmcs_chroma_resid_batch.
Planes are compared whole against the digests; the scale table only on the units whose blocks the host routes to the TB passes.  A failure
names the component and the first differing sample (against the oracle side, which tests/test_ref_recon_cpu.py holds to the same digests);
to find a cause run that test first: with the live reference it stops at the first differing plane.

Before any launch every command list is checked — ref_recon_cases.well_formed (what test_ref_recon_cpu.py accepts) and
vvc355_recon_order_check on the host tables: a malformed order makes the walk wait forever, so nothing unchecked reaches the device."""
import ctypes

import numpy as np
import pytest

import inter_tb_cases as tc
import intra_tb_cases as itc
import levels_cases as lc
import picture_cases as pcs
import recon_cases
import ref_recon_cases as rc
import ts_tb_cases as ts
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

# (how the stages are issued, levels, ticket order)
RUNS = [("entries", "int32", "raster"), ("picture", "int32", "critical"), ("entries", "packed", "critical"), ("picture", "packed", "raster")]


@pytest.fixture(scope="module")
def golden():
    return rc.load_golden()


class DevicePicture:
    """One listed picture in device memory: planes (pitched), arena, records of the three TB passes, scale table, command tables and the
    frames of the five stages."""

    def __init__(self, dev, pic, d, levels, order, shared=None):
        """shared = (arena buffer, inter_tb_cases.DevicePicture) of an inter_tb_cases.OldPath: the picture then lives in those buffers."""
        k = self.k = pcs.Keep()
        self.dev, self.pic, self.d = dev, pic, d
        bd, tp = pic.bd, d.tpic
        n_i, n_e = len(d.intra), len(d.inter)
        offs_i, offs_e, offs_s = d.offs[:n_i], d.offs[n_i:n_i + n_e], d.offs[n_i + n_e:]
        lv = stream = None
        if levels == "packed":
            stream, lv = lc.pack_all([s["c"] for s in d.specs])
            assert not (lv["flags"] & abi.LEVELS_INT32).all(), "no block of the picture is packed"
        self.arena0 = rc.start_arena(d, lv)
        self.d_arena = shared[0] if shared else k.up(self.arena0)
        self.host_planes = shared[1].host if shared else [tc.pitched(p) for p in pic.planes]
        self.d_planes = shared[1].d_planes if shared else [k.up(p) for p in self.host_planes]
        strides = [p.shape[1] * pic.isz for p in self.host_planes]
        d_slice, d_col, d_row = (k.up(a) for a in (pic.slice_idx, pic.col_bd, pic.row_bd))
        d_model = k.up(np.frombuffer(bytes(pic.model), np.uint8))
        d_levels = k.up(stream) if stream is not None else None
        if d_levels is not None:
            assert d_levels.ptr % 32 == 0

        def side(first, n):
            return k.up(lv[first:first + n].view(np.uint8) if n else np.zeros(16, np.uint8)).ptr if lv is not None else 0

        self.scaled = tp.model is not None
        self.table0 = np.full(tp.ux * tp.uy, -1, np.int16)
        self.d_table = shared[1].d_table if shared and self.scaled else k.up(self.table0)
        stages = {}
        if n_i:
            f = abi.IntraTbFrame()
            f.tus, f.coeffs, f.n_tus = k.up(itc.records(d.intra, offs_i).view(np.uint8)).ptr, self.d_arena.ptr, n_i
            for c in range(6):
                f.class_first[c] = d.class_first[c]
            f.range, f.bd = pic.rbits, bd
            f.lv, f.levels = side(0, n_i), d_levels.ptr if d_levels is not None else 0
            stages["intra_tb"] = k.frame(f)
        for name, ty, specs, offs, first, recs, first_lv in (("inter_tb", abi.InterTbFrame, d.inter, offs_e, d.bin_first, tc.records, n_i),
                                                             ("ts_tb", abi.TsTbFrame, d.skip, offs_s, d.ts_first, ts.records, n_i + n_e)):
            if not specs:
                continue
            f = ty()
            f.tus, f.coeffs, f.n_tus = k.up(recs(tp, specs, offs).view(np.uint8)).ptr, self.d_arena.ptr, len(specs)
            for c in range(3):
                f.plane[c], f.stride[c] = self.d_planes[c].ptr, strides[c]
            f.width, f.height, f.hs, f.vs, f.size_y, f.range, f.bd = pic.width, pic.height, pic.hs, pic.vs, pic.size_y, pic.rbits, bd
            f.scale_table = self.d_table.ptr if self.scaled else 0
            dst = f.bin_first if name == "inter_tb" else f.class_first
            for ch in range(2):
                for b in range(len(first[ch])):
                    dst[ch][b] = first[ch][b]
            f.lv, f.levels = side(first_lv, len(specs)), d_levels.ptr if d_levels is not None else 0
            stages[name] = k.frame(f)
        if self.scaled:
            stages["lmcs_scale"] = k.frame(rc.scale_frame(pic, self.d_planes[0].ptr, strides[0], self.d_table.ptr, d_model.ptr, d_slice.ptr, d_col.ptr, d_row.ptr))
        self.order = order
        self.cmds0 = rc.bound_cmds(d, self.d_arena.ptr).view(np.uint8).copy()
        self.d_cmds = k.up(self.cmds0)
        d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(pic.ncx * pic.ncy))
        k.keep.append(d_state)
        stages["recon"] = k.frame(rc.recon_frame(pic, d, [b.ptr for b in self.d_planes], strides, self.d_cmds.ptr, k.up(d.ctus).ptr, k.up(order).ptr,
                                                 d_state.ptr, d_slice.ptr, d_col.ptr, d_row.ptr, d_model.ptr if self.scaled else 0))
        self.stages = stages

    def run_entries(self):
        """The separate entries in INTEGRATION.md's order."""
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
        """One vvc355_picture_pass, the ticket order checked once more by the call itself."""
        ret = pcs.run(self.dev, None, self.pic.bd, pcs.picture(self.stages, recon_tables=(self.d.ctus, self.order)))
        assert ret == 0, f"vvc355_picture_pass refused the picture: stage / code {pcs.decode(ret)}"

    def result(self):
        self.dev.vvc355_stream_sync(None)
        assert self.dev.vvc355_last_error() == 0
        planes = [b.to_host(h.dtype, h.shape) for b, h in zip(self.d_planes, self.host_planes)]
        for c, (g, h, p) in enumerate(zip(planes, self.host_planes, self.pic.planes)):
            assert np.array_equal(g[:, p.shape[1]:], h[:, p.shape[1]:]), f"component {c}: the pitch padding was written"
        table = self.d_table.to_host(np.int16, self.table0.shape) if self.scaled else None
        return [g[:, :p.shape[1]] for g, p in zip(planes, self.pic.planes)], table


def _checked(dev, name, order_kind):
    """The picture, its derived inputs and a ticket order, all checked on the host: nothing else goes to the device."""
    pic = rc.picture(name)
    d = rc.derive(pic)
    bad = rc.well_formed(pic, d)
    assert bad is None, f"{name}: {bad}: not launched"
    order = recon_cases.critical_order(dev, d.ctus, pic.ncx, pic.ncy) if order_kind == "critical" else d.order
    assert rc.order_defect(d.ctus, pic.ncx, pic.ncy, order) is None, f"{name}: not launched"
    assert pcs.order_check(dev, d.ctus, pic.ncx, pic.ncy, order) == 0, f"{name}: vvc355_recon_order_check refuses the {order_kind} order: not launched"
    return pic, d, np.ascontiguousarray(order, np.int32)


def _explain(name, d, planes):
    """The first differing sample, against the oracle side (held to the same digests by the CPU test)."""
    import ref_lib
    want, _t, _a = rc.oracle_side(ref_lib.load_oracle(), d)
    return rc.first_difference(want, planes) or "the oracle side differs from the digests as well: run tests/test_ref_recon_cpu.py"


@pytest.mark.parametrize("how,levels,order_kind", RUNS)
@pytest.mark.parametrize("name", rc.picture_names())
def test_device_reproduces_the_reference_digests(dev, golden, name, how, levels, order_kind):
    pic, d, order = _checked(dev, name, order_kind)
    assert rc.inputs_digest(pic) == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    dp = DevicePicture(dev, pic, d, levels, order)
    (dp.run_entries if how == "entries" else dp.run_picture)()
    planes, table = dp.result()
    got = rc.digests(pic, d, planes, table)
    assert set(got) == set(golden[name])
    bad = sorted(k for k in got if k != "inputs" and got[k] != golden[name][k])
    assert not bad, f"{name} ({how}, {levels} levels, {order_kind} order): {bad} do not hash to the reference's digests: {_explain(name, d, planes)}"


@pytest.mark.parametrize("name", rc.OLD_PATH)
def test_older_job_path_reproduces_the_reference_digests(dev, orc, golden, name):
    """The path the inter record pass replaced, for the transformed blocks of the inter units: vvc355_itx_frame_build, the shape batches, then
    vvc355_lmcs_chroma_resid_batch behind the scale pass (inter_tb_cases.OldPath); the other stages as before."""
    tc.bind_oracle(orc)
    pic, d, order = _checked(dev, name, "raster")
    assert len(pic.slices) == 1 and len(set(pic.col_bd[:-1].tolist())) == 1 and d.inter and not any(s["joint"] & 1 for s in d.inter)
    assert all(d.tpic.unit_of(s, "cu") == d.tpic.unit_of(s, "block") for s in d.inter), "the older path takes the unit from the block's position"
    n_i, n_e = len(d.intra), len(d.inter)
    tcd = tc.DevicePicture(d.tpic)
    old = tc.OldPath(orc, d.tpic, d.inter, d.offs[n_i:n_i + n_e], rc.start_arena(d), pic.rbits, None, dpic=tcd)
    dp = DevicePicture(dev, pic, d, "int32", order, shared=(old.d_arena, tcd))
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
    got = rc.digests(pic, d, planes, table)
    bad = sorted(k for k in got if k != "inputs" and got[k] != golden[name][k])
    assert not bad, f"{name} (older job path): {bad} do not hash to the reference's digests: {_explain(name, d, planes)}"

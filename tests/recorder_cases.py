"""The recorder (include/vvc_mi355_rec.h, ffvvc_amd/host/recorder.c) on the pictures of ref_recon_cases: a picture's flat arrays
(ref_recon_cases.shim_arrays) turned into the recorder's PODs, one run of the recorder with everything it derived copied out, and the
comparison with ref_recon_cases.derive(), which is the restatement of INTEGRATION.md section 3 that the reference's digests hold.

Two things are the recorder's own choice and are normalised before bytes are compared:
  * the arena-slot numbering: record i of the recorder's lists is record i of derive()'s (the lists are compared index by index), so its
    coeff_off is replaced by derive()'s offset of that record; that the recorder's slots are multiples of 4 elements, disjoint and fill
    arena_len exactly is checked apart;
  * a RESID command's `resid`: the recorder puts the slot there, derive() a running number; both become the index of the record they name.
The ticket order is vvc355_recon_order's, where derive() lists the CTUs with commands in raster order: the order is compared with the
helper's answer on derive()'s CTU table, and as a set with derive()'s.

Also: the flat dump tools/recorder_check.c reads, and the digest (FNV-1a, 64 bit) that program prints.
Used by tests/test_recorder_cpu.py, tests/test_recorder_gpu.py and tools/recorder_time.py."""
import ctypes
from types import SimpleNamespace

import numpy as np

import inter_tb_cases as tc
import intra_tb_cases as itc
import levels_cases as lc
import recon_cases
import ref_recon_cases as rc
import ts_tb_cases as ts
from ffvvc_amd import abi

TB, TU, CU = (np.dtype(t, align=True) for t in (abi.RecTb, abi.RecTu, abi.RecCu))
INTRA, INTER, TS = (np.dtype(t, align=True) for t in (abi.IntraTu, abi.InterTu, abi.TsTu))
CMD, CTU, LV = recon_cases.CMD, recon_cases.CTU, lc.LV_DTYPE
SENT = tc.SENT
DUMP_MAGIC = 0x35354352
NO_LEVELS = 0xFFFFFFFFFFFFFFFF


def pods(pic):
    """The picture as the recorder's PODs: SimpleNamespace(first, cus, tus, tbs, levels), pointers set; the arrays must outlive the calls."""
    first, cus, tus, tbs, levels = rc.shim_arrays(pic)
    n_cu, n_tu, n_tb = len(cus), (len(tus) if len(cus) else 0), int(tus["n_tbs"].sum()) if len(cus) else 0
    b = np.zeros(max(n_tb, 1), TB)
    src = tbs[:n_tb]
    for k in ("x0", "y0", "w", "h", "c_idx", "ts", "has_coeffs", "min_x", "min_y", "max_x", "max_y"):
        b[k][:n_tb] = src[k]
    b["levels"][:n_tb] = np.where(src["has_coeffs"] != 0, levels.ctypes.data + 4 * src["level_off"].astype(np.uint64), 0)
    t = np.zeros(max(n_tu, 1), TU)
    src = tus[:n_tu]
    for k in ("x0", "y0", "w", "h", "coded_flag", "n_tbs"):
        t[k][:n_tu] = src[k]
    t["joint_cbcr_residual_flag"][:n_tu] = src["joint"]
    t["tbs"][:n_tu] = b.ctypes.data + TB.itemsize * src["first_tb"].astype(np.uint64)
    c = np.zeros(max(n_cu, 1), CU)
    for k in ("x0", "y0", "w", "h", "pred_mode", "tree_type", "coded_flag", "ciip_flag", "mode_y", "mode_c", "ref_idx", "mip_flag", "mip_mode",
              "mip_transposed", "mip_chroma_direct", "isp_type", "bdpcm", "lfnst_idx", "apply_lfnst", "mts_idx", "sbt_flag", "sbt_horizontal",
              "sbt_pos", "qp", "n_tus"):
        c[k][:n_cu] = cus[k]
    c["tus"][:n_cu] = t.ctypes.data + TU.itemsize * cus["first_tu"].astype(np.uint64)
    return SimpleNamespace(first=first, cus=c, tus=t, tbs=b, levels=levels, n_cu=n_cu, n_tu=n_tu, n_tb=n_tb)


def params(pic, pack=True):
    p = abi.RecParams()
    p.width, p.height, p.ctb_log2, p.bit_depth, p.log2_transform_range, p.chroma_format_idc = pic.width, pic.height, pic.ctb_log2, pic.bd, pic.rbits, pic.idc
    p.qp_bd_offset, p.sps_min_qp_prime_ts = 6 * (pic.bd - 8), pic.min_qp_prime_ts
    p.mts_enabled, p.explicit_mts_intra, p.explicit_mts_inter = pic.mts_enabled, pic.explicit_mts_intra, pic.explicit_mts_inter
    p.ph_joint_cbcr_sign_flag, p.ph_chroma_residual_scale_flag, p.pack_levels = pic.joint_sign, pic.chroma_scale_flag, int(pack)
    return p


def slice_flags(pic, rs):
    dep, lmcs = pic.slices[int(pic.slice_idx[rs])]
    return (abi.REC_SLICE_DEP_QUANT if dep else 0) | (abi.REC_SLICE_LMCS if lmcs else 0)


def feed(lib, rec, pic, p, order=None):
    """vvc355_rec_ctu for the CTUs in `order` (raster by default): the first refusal's code, or 0."""
    for rs in (range(len(pic.ctus)) if order is None else order):
        rs = int(rs)
        if not 0 <= rs < len(pic.ctus):                  # for the refusal tests: an index outside the grid has no units to give
            ret = lib.vvc355_rec_ctu(rec, rs, 0, p.cus.ctypes.data, 0)
            if ret:
                return ret
            continue
        ret = lib.vvc355_rec_ctu(rec, rs, slice_flags(pic, rs), p.cus.ctypes.data + CU.itemsize * int(p.first[rs]), int(p.first[rs + 1] - p.first[rs]))
        if ret:
            return ret
    return 0


def _copy(ptr, n, dtype):
    dtype = np.dtype(dtype)
    return np.frombuffer(ctypes.string_at(ptr, n * dtype.itemsize), dtype).copy() if n else np.zeros(0, dtype)


def snapshot(lib, rec, res):
    """Everything a vvc355_rec_result names, copied out, and the arena after vvc355_rec_fill_arena on sentinels."""
    o = SimpleNamespace(res=res, head=bytes(res)[abi.RecResult.n_levels.offset:abi.RecResult.late_keep.offset])
    o.cmds, o.ctus, o.order = _copy(res.cmds, res.n_cmds, CMD), _copy(res.ctus, res.n_ctus, CTU), _copy(res.order, res.n_work, np.int32)
    o.intra, o.inter, o.ts = _copy(res.intra, res.n_intra, INTRA), _copy(res.inter, res.n_inter, INTER), _copy(res.ts, res.n_ts, TS)
    o.lv = np.concatenate([_copy(p, n, LV) for p, n in ((res.intra_lv, res.n_intra), (res.inter_lv, res.n_inter), (res.ts_lv, res.n_ts))])
    o.levels = _copy(res.levels, res.n_levels, np.int16)
    o.class_first = list(res.class_first)
    o.bin_first, o.ts_first = [list(r) for r in res.bin_first], [list(r) for r in res.ts_first]
    o.n_work, o.arena_len = res.n_work, int(res.arena_len)
    o.stats = dict(keep=res.keep, batched_scaled=res.batched_scaled, walk_scaled=res.walk_scaled)
    o.late_keep = res.late_keep
    o.arena = np.full(o.arena_len, SENT, np.int32)
    assert lib.vvc355_rec_fill_arena(rec, o.arena.ctypes.data if o.arena_len else np.zeros(1, np.int32).ctypes.data) == 0
    return o


def record(lib, pic, pack=True, order=None, rec=None, p=None):
    """One picture through the recorder (a fresh object unless `rec` is given, which is then left ended and alive): the snapshot."""
    own = rec is None
    rec = lib.vvc355_rec_create() if own else rec
    try:
        p = pods(pic) if p is None else p
        par = params(pic, pack)
        assert lib.vvc355_rec_begin_picture(rec, ctypes.byref(par)) == 0
        ret = feed(lib, rec, pic, p, order)
        assert ret == 0, f"{pic.name}: vvc355_rec_ctu refused a CTU: {ret}"
        res = abi.RecResult()
        assert lib.vvc355_rec_end_picture(rec, ctypes.byref(res)) == 0
        return snapshot(lib, rec, res)
    finally:
        if own:
            lib.vvc355_rec_destroy(rec)


def slots(o):
    """coeff_off of the recorder's records in list order (intra, inter, ts) and their sizes in elements."""
    off = np.concatenate([o.intra["coeff_off"], o.inter["coeff_off"], o.ts["coeff_off"]]).astype(np.int64)
    size = np.concatenate([np.int64(1) << (r["log2_w"].astype(np.int64) + r["log2_h"]) for r in (o.intra, o.inter, o.ts)])
    return off, size


def slot_defect(o):
    """None, or what is wrong with the recorder's slot numbering."""
    off, size = slots(o)
    if np.any(off % 4):
        return "a slot that is not a multiple of 4 elements"
    k = np.argsort(off, kind="stable")
    ends = off[k] + ((size[k] + 3) & ~3)
    if len(off) and (np.any(ends[:-1] > off[k][1:]) or ends[-1] > o.arena_len):
        return "slots overlap or leave the arena"
    return None if int(((size + 3) & ~3).sum()) == o.arena_len else "arena_len is not the sum of the slots"


def differences(lib, pic, d, o, pack):
    """What of the recorder's output differs from derive()'s, by name; [] = byte for byte equal (after the two normalisations)."""
    bad = []

    def cmp(name, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.dtype != want.dtype or got.shape != want.shape or got.tobytes() != want.tobytes():
            bad.append(name)

    n_i, n_e, n_s = len(d.intra), len(d.inter), len(d.skip)
    if (len(o.intra), len(o.inter), len(o.ts)) != (n_i, n_e, n_s):
        return [f"list lengths {(len(o.intra), len(o.inter), len(o.ts))} against {(n_i, n_e, n_s)}"]
    defect = slot_defect(o)
    if defect:
        bad.append(defect)
    off, size = slots(o)
    offs = np.array(d.offs, np.int64)
    # records, in derive()'s slot numbering
    for name, got, first, n, want in (("intra", o.intra, 0, n_i, itc.records(d.intra, d.offs[:n_i])),
                                      ("inter", o.inter, n_i, n_e, tc.records(d.tpic, d.inter, d.offs[n_i:n_i + n_e])),
                                      ("ts", o.ts, n_i + n_e, n_s, ts.records(d.tpic, d.skip, d.offs[n_i + n_e:]))):
        g = got.copy()
        g["coeff_off"] = offs[first:first + n]
        cmp(name + " records", g.view(np.uint8), np.ascontiguousarray(want).view(np.uint8).reshape(-1)[:16 * n])
    cmp("class_first", np.array(o.class_first), np.array(d.class_first))
    cmp("bin_first", np.array(o.bin_first), np.array(d.bin_first))
    cmp("ts_first", np.array(o.ts_first), np.array(d.ts_first))
    # commands: resid -> the record it names
    index_of_slot = {int(s): i for i, s in enumerate(off)}
    index_of_rid = {s["rid"]: i for i, s in enumerate(d.specs)}
    got, want = o.cmds.copy(), d.cmds.copy()
    try:
        is_res = got["kind"] == abi.RECON_RESID
        got["resid"][is_res] = [index_of_slot[int(v)] for v in got["resid"][is_res]]
        is_res = want["kind"] == abi.RECON_RESID
        want["resid"][is_res] = [index_of_rid[int(v)] for v in want["resid"][is_res]]
        cmp("commands", got.view(np.uint8), want.view(np.uint8))
    except KeyError:
        bad.append("a RESID command names no record's slot")
    cmp("CTU table", o.ctus.view(np.uint8), np.ascontiguousarray(d.ctus).view(np.uint8))
    if o.n_work != len(d.order) or sorted(o.order.tolist()) != d.order.tolist():
        bad.append("n_work / the CTUs in the order")
    cmp("ticket order", o.order, recon_cases.critical_order(lib, d.ctus, pic.ncx, pic.ncy))
    # levels
    stream, lv = lc.pack_all([s["c"] for s in d.specs], force_int32=() if pack else set(range(len(d.specs))))
    cmp("side records", o.lv.view(np.uint8), lv.view(np.uint8))
    cmp("level stream", o.levels, stream)
    # the arena after fill_arena, in derive()'s numbering
    arena = np.full(d.arena_len, SENT, np.int32)
    covered = np.zeros(o.arena_len, bool)
    for i in range(len(off)):
        arena[offs[i]:offs[i] + size[i]] = o.arena[off[i]:off[i] + size[i]]
        covered[off[i]:off[i] + size[i]] = True
    cmp("arena", arena, rc.start_arena(d, lv))
    if np.any(o.arena[~covered] != SENT):
        bad.append("fill_arena wrote outside the slots")
    if o.stats != {k: int(v) for k, v in d.stats.items()}:
        bad.append(f"statistics {o.stats} against {d.stats}")
    return bad


# ---------------------------------------------------------------------------------------------------------------- the stand-alone check

def fnv1a(*chunks):
    h = 0xCBF29CE484222325
    for c in chunks:
        for v in bytes(c):
            h = ((h ^ v) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def digest(o):
    """What tools/recorder_check.c prints for a run: everything derived but the ticket order (that program has no vvc355_recon_order) and
    late_keep (it depends on the order of the calls)."""
    return fnv1a(o.head, o.cmds.view(np.uint8), o.ctus.view(np.uint8), o.intra.view(np.uint8), o.inter.view(np.uint8), o.ts.view(np.uint8),
                 o.lv.view(np.uint8), o.levels.view(np.uint8), o.arena.view(np.uint8))


def dump(pic, path, pack=True):
    """The flat dump of a picture's PODs: int32 header (magic, CTUs, units, transform units, blocks, levels), vvc355_rec_params, first unit
    per CTU (+1), slice flags per CTU, then the three POD arrays with indices in place of pointers (NO_LEVELS = none) and the int32 levels."""
    p = pods(pic)
    first, cus, tus, tbs, levels = rc.shim_arrays(pic)
    c, t, b = p.cus[:p.n_cu].copy(), p.tus[:p.n_tu].copy(), p.tbs[:p.n_tb].copy()
    c["tus"], t["tbs"] = cus["first_tu"], tus[:p.n_tu]["first_tb"]
    b["levels"] = np.where(tbs[:p.n_tb]["has_coeffs"] != 0, tbs[:p.n_tb]["level_off"].astype(np.uint64), np.uint64(NO_LEVELS))
    with open(path, "wb") as f:
        f.write(np.array([DUMP_MAGIC, len(pic.ctus), p.n_cu, p.n_tu, p.n_tb, len(levels)], np.int32).tobytes())
        f.write(bytes(params(pic, pack)))
        f.write(first.astype(np.int32).tobytes())
        f.write(np.array([slice_flags(pic, rs) for rs in range(len(pic.ctus))], np.int32).tobytes())
        for a in (c, t, b, levels.astype(np.int32)):
            f.write(a.tobytes())

"""CPU: the oracle's in-loop filter passes — orc_deblock_bs_pass, orc_deblock_frame_pass (vertical, then horizontal), orc_sao_frame_pass,
orc_alf_frame_pass — against the reference's own callers on whole pictures (oracle/ref_shim_filter.c).

* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): every listed picture and a sweep of freshly drawn ones, tables and
  planes compared whole.
* Digests (everywhere): the oracle reproduces tests/golden/ref_passes.json, and the generator still hashes to the recorded inputs.
* Premises (everywhere): what the listed pictures must exercise, counted from the inputs and the reference's outputs with the index
  arithmetic restated in numpy.  Where the library is absent the reference's outputs are the oracle's, after they hashed to the
  reference's digests."""
import os
import sys
import time
from collections import Counter

import numpy as np
import pytest

import ref_lib
import ref_pass_cases as pc

SWEEP = 64                                     # pictures per family; the sweep asserts that many were compared


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load()


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


def _compare_deblock(ref, orc, pic):
    want, got = pc.run_deblock(ref, "ref", pic), pc.run_deblock(orc, "orc", pic)
    lines = pc.table_differences(pic, want, got)
    for s in ("v", "h"):
        lines += pc.plane_differences(pic.name, s, want[s], got[s])
    assert not lines, "\n".join(lines)


def _compare_filter(ref, orc, fp):
    for s in ("sao", "alf"):
        lines = pc.plane_differences(fp.name, s, pc.run_filter(ref, "ref", fp, s), pc.run_filter(orc, "orc", fp, s))
        assert not lines, "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", pc.DEBLOCK)
def test_live_deblocking_equals_the_reference(ref, orc, name):
    _need(ref)
    _compare_deblock(ref, orc, pc.deblock_picture(orc, name))


@pytest.mark.parametrize("name", pc.FILTER)
def test_live_sao_and_alf_equal_the_reference(ref, orc, name):
    _need(ref)
    _compare_filter(ref, orc, pc.filter_picture(name))


def test_live_chain_equals_the_reference(ref, orc):
    _need(ref)
    d, _ = pc.chain_picture()
    want, got = pc.run_chain(ref, "ref"), pc.run_chain(orc, "orc")
    lines = pc.table_differences(d, want, got)
    for s in ("v", "h", "sao", "alf"):
        lines += pc.plane_differences(pc.CHAIN, s, want[s], got[s])
    assert not lines, "\n".join(lines)


def test_live_alf_mapping_carries_the_generators_sets(ref):
    _need(ref)
    assert ref.ref_alf_luma_sets() == pc.ALF_LUMA_SETS


def test_live_sweep_deblocking(ref, orc):
    _need(ref)
    t0, seen, n = time.time(), Counter(), 0
    for k in range(SWEEP):
        pic = pc.sweep_deblock(k)
        _compare_deblock(ref, orc, pic)
        seen[(pic.bd, pic.n_comp, pic.t.hs, pic.t.vs, pic.t.ctb_log2, pic.min_cb_log2, bool(pic.ladf))] += 1
        n += 1
    assert n >= 64, n
    assert {k[0] for k in seen} == {8, 10, 12} and {k[4] for k in seen} == {5, 6, 7} and {k[1] for k in seen} == {1, 3} and {k[5] for k in seen} == {2, 3}
    print(f"{n} deblocking pictures in {len(seen)} configurations compared in {time.time() - t0:.1f} s")


def test_live_sweep_sao_and_alf(ref, orc):
    _need(ref)
    t0, seen, n = time.time(), Counter(), 0
    for k in range(SWEEP):
        fp = pc.sweep_filter(k)
        _compare_filter(ref, orc, fp)
        seen[(fp.bd, fp.n_comp, fp.t.hs, fp.t.vs, fp.t.ctb_log2, fp.lfase, fp.lfate)] += 1
        n += 1
    assert n >= 64, n
    assert {k[0] for k in seen} == {8, 10, 12} and {k[4] for k in seen} == {5, 6, 7} and {k[1] for k in seen} == {1, 3}
    assert {(k[5], k[6]) for k in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    print(f"{n} SAO / ALF pictures in {len(seen)} configurations compared in {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------- digests

@pytest.mark.parametrize("name", pc.picture_names())
def test_oracle_reproduces_reference_digests(golden, orc, ref, name):
    assert name in golden, f"{name} is not in ref_passes.json: regenerate it (tests/golden/README.md)"
    got = pc.host_digests(orc, orc, "orc", name)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the unit or sample")


def test_no_picture_left_out(golden):
    assert list(golden) == pc.picture_names()


def test_fixture_is_fresh(ref, orc):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(pc.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_passes(ref, orc)), "tests/golden/ref_passes.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- premises

def _reference_run(orc, ref, golden, name):
    """(inputs, outputs of the reference) of a listed picture.  Without the library: the oracle's outputs, once they hash to the reference's."""
    lib, side = (ref, "ref") if ref is not None else (orc, "orc")
    if ref is None:
        got = pc.host_digests(orc, orc, "orc", name)
        assert got == golden[name], f"{name}: the oracle does not reproduce the reference's digests"
    if name == pc.CHAIN:
        return pc.chain_picture(), pc.run_chain(lib, side)
    if name in pc.DEBLOCK:
        pic = pc.deblock_picture(orc, name)
        return pic, pc.run_deblock(lib, side, pic)
    fp = pc.filter_picture(name)
    return fp, {s: pc.run_filter(lib, side, fp, s) for s in ("sao", "alf")}


def _p_side(a, d):
    """a[r, c - 1] (d = 1: vertical edges, the P side is the unit on the left) or a[r - 1, c] (d = 0); the first column / row repeats itself."""
    return np.concatenate([a[:, :1], a[:, :-1]], 1) if d else np.concatenate([a[:1], a[:-1]], 0)


def _deblock_premises(pic, out, n):
    """Counts into `n` from one deblocking picture: `out` = the reference's tables and planes."""
    t, a = pic.t, pic.arrays
    ctb, log2 = 1 << t.ctb_log2, t.ctb_log2
    X, Y = np.broadcast_to(4 * np.arange(t.tw)[None, :], (t.th, t.tw)), np.broadcast_to(4 * np.arange(t.th)[:, None], (t.th, t.tw))
    rs = (Y >> log2) * t.cw + (X >> log2)
    slice_u = t.slice_idx[rs].astype(int)
    col_u, row_u = t.col_bd[X >> log2], t.row_bd[Y >> log2]
    mcl = pic.min_cb_log2
    qpy_u = a["qp_y"][Y >> mcl, X >> mcl].astype(int)
    mvf, dbp = t.mvf, a["dbp"].astype(int)
    pf, ciip, ridx = mvf["pred_flag"].astype(int), mvf["ciip_flag"].astype(int), mvf["ref_idx"].astype(int)
    qp_bd = 6 * (pic.bd - 8)
    planes_before = {1: pic.planes, 0: out["v"]}
    planes_after = {1: out["v"], 0: out["h"]}
    for d in (0, 1):
        pos = X if d else Y
        on_ctu = (pos > 0) & (pos % ctb == 0)
        bs_l = out[f"bs{d}0"].astype(int)
        # (1) every strength in every table at grid positions; (2) every filter length
        for c in range(pic.n_comp):
            tab, mask = out[f"bs{d}{c}"], pc.read_mask(pic, f"bs{d}{c}")
            for v in (0, 1, 2):
                n[f"bs{d}{c}=={v}"] += int(np.count_nonzero(tab[mask] == v))
        live = pc.read_mask(pic, f"bs{d}0") & (bs_l > 0)
        for side in "pq":
            for v in (1, 2, 3, 5, 7):
                n[f"{side}{d}=={v}"] += int(np.count_nonzero(out[f"{side}{d}"][live] == v))
        # (3) a slice edge between two inter units without coded flags whose slices' POC lists differ at the indices used
        sl_p, pf_p, ridx_p = _p_side(slice_u, d), _p_side(pf, d), _p_side(ridx, d)
        tile_edge = on_ctu & ((col_u if d else row_u) != _p_side(col_u if d else row_u, d))
        slice_edge = on_ctu & (slice_u != sl_p)
        filtered = (~slice_edge | bool(t.lfase)) & (~tile_edge | bool(t.lfate))
        motion = (pf > 0) & (pf_p > 0) & (ciip == 0) & (_p_side(ciip, d) == 0) & (a["cbf0"] == 0) & (_p_side(a["cbf0"], d) == 0) & \
                 ~((a["pcm0"] != 0) & (_p_side(a["pcm0"], d) != 0))
        lists_differ = np.zeros(pf.shape, bool)
        for lst in (0, 1):
            for flags, idx in ((pf, ridx[..., lst]), (pf_p, ridx_p[..., lst])):
                used = (flags >> lst) & 1
                lists_differ |= (used == 1) & (t.ref_poc[slice_u, lst, idx] != t.ref_poc[sl_p, lst, idx])
        n["slice edge, motion rule, POC lists differ"] += int(np.count_nonzero(slice_edge & filtered & motion & lists_differ))
        # (4) CTU edges of slices and tiles: suppressed with the flag off (an intra side would have made it 2), filtered with it on
        intra = (pf == 0) | (pf_p == 0)
        both_pcm = (a["pcm0"] != 0) & (_p_side(a["pcm0"], d) != 0)
        if not t.lfase:
            assert not np.any(bs_l[slice_edge]), f"{pic.name}: a slice edge is filtered with lfase = 0"
            n["slice edge suppressed"] += int(np.count_nonzero(slice_edge & intra & ~both_pcm))
        else:
            n["slice edge filtered"] += int(np.count_nonzero(slice_edge & filtered & (bs_l > 0)))
        if not t.lfate:
            assert not np.any(bs_l[tile_edge]), f"{pic.name}: a tile edge is filtered with lfate = 0"
            n["tile edge suppressed"] += int(np.count_nonzero(tile_edge & intra & ~both_pcm))
        else:
            n["tile edge filtered"] += int(np.count_nonzero(tile_edge & filtered & (bs_l > 0)))
        # (7, 8) luma: LADF interval, beta and tc index before the clip.  The level is read from the planes as they are BEFORE the pass; the
        # reference reads samples that earlier edges of the same pass may have filtered, so single units can fall in the neighbouring interval.
        luma = planes_before[d][0].astype(int)
        if d:
            xs = np.maximum(X, 1)
            level = (luma[Y, xs - 1] + luma[Y + 3, xs - 1] + luma[Y, xs] + luma[Y + 3, xs]) >> 2
        else:
            ys = np.maximum(Y, 1)
            level = (luma[ys - 1, X] + luma[ys - 1, X + 3] + luma[ys, X] + luma[ys, X + 3]) >> 2
        qp = (qpy_u + _p_side(qpy_u, d) + 1) >> 1
        if pic.ladf:
            interval = sum((level > b).astype(int) for b in pic.ladf["bounds"][1:])
            qp = qp + np.array([pic.ladf["lowest"]] + pic.ladf["offsets"])[interval]
            for k in range(5):
                n[f"LADF interval {k}"] += int(np.count_nonzero(live & (interval == k)))
        beta_i, tc_i = qp + dbp[rs, 0], qp + 2 * (bs_l - 1) + (dbp[rs, 3] & -2)
        for key, m in (("luma beta < 0", beta_i < 0), ("luma beta > 63", beta_i > 63), ("luma tc < 0", tc_i < 0), ("luma tc > 65", tc_i > 65)):
            n[key] += int(np.count_nonzero(live & m))
        # (9) the long filters ran: a changed luma sample four or more away from the nearest filtered edge of its line
        changed = planes_before[d][0] != planes_after[d][0]
        edges = bs_l > 0
        if not d:
            changed, edges = changed.T, edges.T
        x = np.arange(changed.shape[1])[:, None]
        for r in range(edges.shape[0]):
            xe = 4 * np.nonzero(edges[r])[0][None, :]
            if xe.size:
                dist = np.where(x >= xe, x - xe, xe - 1 - x).min(1)
                n[f"dir {d}: changed luma sample >= 4 from its edge"] += int(np.count_nonzero(changed[4 * r:4 * r + 4].any(0) & (dist >= 4)))
        # (10) every component changed in both passes
        for c in range(pic.n_comp):
            assert np.any(planes_before[d][c] != planes_after[d][c]), f"{pic.name}: component {c} unchanged by the {'vertical' if d else 'horizontal'} pass"
        if pic.n_comp < 3:
            continue
        # (5, 6, 8) chroma
        size = a["tbw1"] if d else a["tbh1"]
        size_p = _p_side(size, d)
        for c in (1, 2):
            bs_c = out[f"bs{d}{c}"].astype(int)
            grid = pc.read_mask(pic, f"bs{d}{c}") & (bs_c > 0)
            big = (size >= 8) & (size_p >= 8)
            if not d:
                n["chroma horizontal CTU edge, both sizes >= 8"] += int(np.count_nonzero(grid & on_ctu & big))
            n["chroma edge beside a block under 8, bS 2"] += int(np.count_nonzero(grid & ~big & (bs_c == 2)))
            n["chroma edge beside a block under 8, bS 1"] += int(np.count_nonzero(grid & ~big & (bs_c == 1)))
            qc = a[f"qp_c{c - 1}"].astype(int)
            qp = (qc + _p_side(qc, d) - 2 * qp_bd + 1) >> 1
            beta_i, tc_i = qp + dbp[rs, c], qp + 2 * (bs_c - 1) + (dbp[rs, 3 + c] & -2)
            for key, m in (("chroma beta < 0", beta_i < 0), ("chroma beta > 63", beta_i > 63), ("chroma tc < 0", tc_i < 0), ("chroma tc > 65", tc_i > 65)):
                n[key] += int(np.count_nonzero(grid & m))


def _filter_premises(fp, before, out, n):
    t = fp.t
    sao, alf = fp.sao.reshape(-1, 40), fp.alf.reshape(-1, 8)
    sl = t.slice_idx.reshape(t.ch, t.cw).astype(int)
    for stage in ("sao", "alf"):
        for c in range(fp.n_comp):
            assert np.any(before[stage][c] != out[stage][c]), f"{fp.name}: component {c} unchanged by {stage}"
    for yc in range(t.ch):
        for xc in range(t.cw):
            rs = yc * t.cw + xc
            kinds = []
            if not fp.lfase:
                kinds += ["slice, vertical"] * int((xc > 0 and sl[yc, xc - 1] != sl[yc, xc]) or (xc + 1 < t.cw and sl[yc, xc + 1] != sl[yc, xc]))
                kinds += ["slice, horizontal"] * int((yc > 0 and sl[yc - 1, xc] != sl[yc, xc]) or (yc + 1 < t.ch and sl[yc + 1, xc] != sl[yc, xc]))
            if fp.no_tile_filter:
                kinds += ["tile, vertical"] * int((xc > 0 and t.col_bd[xc] == xc) or (xc + 1 < t.cw and t.col_bd[xc] != t.col_bd[xc + 1]))
                kinds += ["tile, horizontal"] * int((yc > 0 and t.row_bd[yc] == yc) or (yc + 1 < t.ch and t.row_bd[yc] != t.row_bd[yc + 1]))
            for c in range(fp.n_comp):
                ty = int(sao[rs, 30 + c])                       # abi.SaoCtb: offset_val int16 [3][5], then type_idx[3]
                for kind in kinds:
                    if ty:
                        n[f"SAO {'band' if ty == 1 else 'edge'} at a restricted edge ({kind})"] += 1
            if alf[rs, 0]:
                n["ALF luma, fixed set" if alf[rs, 3] < 16 else "ALF luma, APS set"] += 1
            if fp.n_comp == 3:
                for c in range(2):
                    n[f"ALF cc_idc[{c}] == {int(alf[rs, 6 + c])}"] += 1
                n["ALF cc on Cr in a slice without a Cr APS"] += int(sl[yc, xc] == 1 and alf[rs, 7] > 0)


PREMISES = ([f"bs{d}{c}=={v}" for d in (0, 1) for c in (0, 1, 2) for v in (0, 1, 2)] +
            [f"{s}{d}=={v}" for s in "pq" for d in (0, 1) for v in (1, 2, 3, 5, 7)] +
            ["slice edge, motion rule, POC lists differ", "slice edge suppressed", "slice edge filtered", "tile edge suppressed", "tile edge filtered",
             "chroma horizontal CTU edge, both sizes >= 8", "chroma edge beside a block under 8, bS 2", "chroma edge beside a block under 8, bS 1"] +
            [f"LADF interval {k}" for k in range(5)] +
            [f"{c} {q}" for c in ("luma", "chroma") for q in ("beta < 0", "beta > 63", "tc < 0", "tc > 65")] +
            [f"dir {d}: changed luma sample >= 4 from its edge" for d in (0, 1)] +
            [f"SAO {ty} at a restricted edge ({k}, {o})" for ty in ("band", "edge") for k in ("slice", "tile") for o in ("vertical", "horizontal")] +
            ["ALF luma, fixed set", "ALF luma, APS set", "ALF cc on Cr in a slice without a Cr APS"] + [f"ALF cc_idc[{c}] == {v}" for c in (0, 1) for v in range(5)])


def test_premises_of_the_listed_pictures(orc, ref, golden):
    t0, n = time.time(), Counter()
    for name in pc.DEBLOCK:
        pic, out = _reference_run(orc, ref, golden, name)
        _deblock_premises(pic, out, n)
    for name in pc.FILTER:
        fp, out = _reference_run(orc, ref, golden, name)
        _filter_premises(fp, {"sao": fp.planes, "alf": fp.planes}, out, n)
    (d, fp), out = _reference_run(orc, ref, golden, pc.CHAIN)
    _deblock_premises(d, out, n)
    _filter_premises(fp, {"sao": out["h"], "alf": out["sao"]}, out, n)
    for key in PREMISES:
        print(f"{key}: {n[key]}")
    missing = [key for key in PREMISES if n[key] <= 0]
    assert not missing, f"premises that hold nowhere in the list: {missing}"
    assert set(n) <= set(PREMISES), sorted(set(n) - set(PREMISES))
    print(f"{len(PREMISES)} premises hold, counted in {time.time() - t0:.1f} s")

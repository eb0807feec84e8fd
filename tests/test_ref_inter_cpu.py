"""CPU: the oracle's inter prediction passes — orc_inter_frame_pass; the job arrays of affine_gpm_cases.expect_affine / expect_gpm through
orc_affine_block / orc_bipred_block / orc_gpm_block; ciip_frame_cases' restatement of the CIIP builder — against the reference's own callers
on whole pictures (oracle/ref_shim_inter.c: ff_vvc_predict_inter, ff_vvc_predict_ciip).

* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): every listed picture and a sweep of freshly drawn ones per driver kind,
  planes, tab_dmvr_mvf, CIIP scratch and intra weights compared whole.
* Digests (everywhere): the oracle side reproduces tests/golden/ref_inter.json, and the generator still hashes to the recorded inputs.
* Premises (everywhere): what the listed pictures must exercise, counted from the inputs, from tab_dmvr_mvf as the reference wrote it
  (the oracle's, after it hashed to the reference's digest, where the library is absent) and — the SAD of the DMVR search, which no output
  of the reference shows — from the oracle's records, which the live comparison and the digests hold to the reference's refined motion."""
import os
import sys
import time
from collections import Counter, defaultdict

import numpy as np
import pytest

import ciip_frame_cases as cc
import ref_inter_cases as ic
import ref_lib

SWEEP = 48                                     # pictures per driver kind; the sweep asserts that many were compared


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load()


@pytest.fixture(scope="module")
def golden():
    return ic.load_golden()


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


def test_reference_library_is_built_where_the_tree_is():
    tree = ref_lib.reference_tree()
    if tree is None:
        pytest.skip("no reference tree on this machine")
    lib = ref_lib.load()
    assert lib is not None, f"the reference tree is at {tree} but {ref_lib.LIB_PATH} is missing: `make -C oracle ref` fails (see stderr)"
    for entry in ("ref_inter_picture", "ref_affine_picture", "ref_gpm_picture", "ref_ciip_picture"):
        assert hasattr(lib, entry), f"{ref_lib.LIB_PATH} has no {entry}: oracle/ref_shim_inter.c is not part of it"


def _compare(ref, orc, pic):
    want, got = ic.run_picture(ref, "ref", pic), ic.run_picture(orc, "orc", pic)
    lines = ic.plane_differences(pic, want.planes, got.planes)
    if "R" in pic.kinds:
        lines += ic.dmvr_differences(pic, want.dmvr, got.dmvr)
    assert not lines, "\n".join(lines)
    for c, p in enumerate(want.planes):
        outside = ~pic.covered[::1 << (pic.vs if c else 0), ::1 << (pic.hs if c else 0)]
        assert (p[outside] == pic.sentinel).all(), f"{pic.name}: component {c}: the reference wrote outside every unit"
    return want, got


def _compare_ciip(ref, orc, cp):
    want, got = ic.run_ciip(ref, "ref", cp), ic.run_ciip(orc, "orc", cp)
    lines = ic.ciip_differences(cp, want, got)
    assert not lines, "\n".join(lines)
    assert (want.scratch[~cc.region_mask(cp.p)] == cp.sentinel).all(), f"{cp.name}: the reference wrote between the units' regions"
    for c in range(cp.n_comp):
        keep = ~cc.plane_mask(cp.p, c) if c else np.ones_like(want.planes[0], bool)
        assert (want.planes[c][keep] == cp.sentinel).all(), f"{cp.name}: component {c}: the reference wrote to the plane beside the 2-wide chroma blocks"
    return want


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", ic.REGULAR + ic.AFFINE + ic.GPM + [ic.MIXED])
def test_live_prediction_equals_the_reference(ref, orc, name):
    _need(ref)
    _compare(ref, orc, ic.picture(name))


@pytest.mark.parametrize("name", ic.CIIP)
def test_live_ciip_equals_the_reference(ref, orc, name):
    _need(ref)
    _compare_ciip(ref, orc, ic.ciip_picture(name))


@pytest.mark.parametrize("kind", ["R", "A", "G"])
def test_live_sweep(ref, orc, kind):
    _need(ref)
    t0, seen, n, units = time.time(), Counter(), 0, 0
    for k in range(SWEEP):
        pic = ic.sweep_picture(kind, k)
        _compare(ref, orc, pic)
        seen[(pic.bd, pic.idc, pic.ctb_log2)] += 1
        units += len(pic.units)
        n += 1
    assert n >= 48, n
    assert {k[0] for k in seen} == {8, 10, 12} and {k[2] for k in seen} == {5, 6, 7} and {k[1] for k in seen} == ({1, 2, 3} if kind == "G" else {0, 1, 2, 3})
    print(f"{n} {kind} pictures ({units} units) in {len(seen)} configurations compared in {time.time() - t0:.1f} s")


def test_live_sweep_ciip(ref, orc):
    _need(ref)
    t0, seen, n, units = time.time(), Counter(), 0, 0
    for k in range(SWEEP):
        cp = ic.sweep_ciip(k)
        _compare_ciip(ref, orc, cp)
        seen[(cp.bd, cp.p.idc, cp.p.ctb_log2)] += 1
        units += len(cp.p.cus)
        n += 1
    assert n >= 48, n
    assert {k[0] for k in seen} == {8, 10, 12} and {k[2] for k in seen} == {5, 6, 7} and {k[1] for k in seen} == {0, 1, 2, 3}
    print(f"{n} CIIP pictures ({units} units) in {len(seen)} configurations compared in {time.time() - t0:.1f} s")


def test_shim_refuses_slices_inside_a_ctu(ref):
    """Two units of one CTU that name different slices: the reference keeps one SliceContext per CTU."""
    _need(ref)
    pic = ic.sweep_picture("R", 0)
    rs = lambda p: (int(p["y0"]) >> pic.ctb_log2, int(p["x0"]) >> pic.ctb_log2)          # noqa: E731
    pair = [i for i in range(1, len(pic.pus)) if rs(pic.pus[i]) == rs(pic.pus[i - 1])]
    assert pair
    saved = int(pic.pus[pair[0]]["slice"])
    pic.pus[pair[0]]["slice"] = (saved + 1) % 3
    with pytest.raises(AssertionError, match="refused"):
        ic.run_picture(ref, "ref", pic)
    pic.pus[pair[0]]["slice"] = saved
    ic.run_picture(ref, "ref", pic)


# ---------------------------------------------------------------------------------------------------------------- digests

@pytest.mark.parametrize("name", ic.picture_names())
def test_oracle_reproduces_reference_digests(golden, orc, ref, name):
    assert name in golden, f"{name} is not in ref_inter.json: regenerate it (tests/golden/README.md)"
    got = ic.host_digests(orc, "orc", name)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the unit or sample")


def test_no_picture_left_out(golden):
    assert list(golden) == ic.picture_names()


def test_fixture_is_fresh(ref):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(ic.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_inter(ref)), "tests/golden/ref_inter.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- premises

def _phases(ph, idc, hs, vs, chroma, mvx, mvy, luma=True):
    if luma:
        ph[(idc, "luma x")].add(mvx & 15)
        ph[(idc, "luma y")].add(mvy & 15)
    if chroma:
        ph[(idc, "chroma x")].add((mvx & ((16 << hs) - 1)) << (1 - hs))         # chroma_mc*: av_mod_uintp2(mv, 4 + shift) << (1 - shift)
        ph[(idc, "chroma y")].add((mvy & ((16 << vs) - 1)) << (1 - vs))


def _regular_premises(pic, out, dmvr, n, ph, shapes):
    """out: the oracle's run (job arrays, records); dmvr: tab_dmvr_mvf as the reference wrote it."""
    jl, rec = out.jl, out.rec
    counts = [ic.ifc.n_jobs_of(p["cb_width"], p["cb_height"], p["num_sb_x"], p["num_sb_y"]) for p in pic.pus]
    pu_of = np.repeat(np.arange(len(pic.pus)), counts)
    W, H = pic.width, pic.height
    for p in pic.pus:
        w, h, d, b = int(p["cb_width"]), int(p["cb_height"]), int(p["dmvr_flag"]), int(p["bdof_flag"])
        uni = int(pic.mvf[int(p["y0"]) >> 2, int(p["x0"]) >> 2]["pred_flag"]) != 3
        shapes.add((w, h, "uni" if uni else "flags" if d or b else "plain"))
        n["hpel_if_idx 1" if p["hpel_if_idx"] else "hpel_if_idx 0"] += 1
        n["BDOF alone"] += int(b and not d)
        n["DMVR alone"] += int(d and not b)
        n["DMVR and BDOF"] += int(d and b)
        n["sub-block merge unit, 8x8 sub-blocks"] += int(not d and not b and p["num_sb_x"] * p["num_sb_y"] > 1 and w // p["num_sb_x"] == 8)
        n[f"regular unit in a slice with LMCS {'on' if pic.slices[int(p['slice'])].lmcs_used else 'off'}"] += 1
    for i in range(len(jl)):
        j, r, pu = jl[i], rec[i], pic.pus[pu_of[i]]
        pf, sl = int(j["pred_flag"]), int(pu["slice"])
        x, y, w, h = (int(j[k]) for k in ("x", "y", "w", "h"))
        for l in range(2):
            if not pf & (1 << l):
                continue
            mvx, mvy = int(r[2 * l]), int(r[2 * l + 1])            # the motion the block is predicted at (refined where DMVR ran)
            _phases(ph, pic.idc, pic.hs, pic.vs, pic.chroma, mvx, mvy)
            ox, oy = x + (mvx >> 4), y + (mvy >> 4)
            if ox + w <= 0 or ox >= W or oy + h <= 0 or oy >= H:
                n["motion wholly outside the picture"] += 1
                continue
            side = ("top" if oy < 0 else "bottom" if oy + h > H else "") + ("left" if ox < 0 else "right" if ox + w > W else "")
            if side:
                n[f"motion leaves the picture: {side}"] += 1
        if pf == 3:
            if j["weight_flag"] and j["denom"] == 2:
                n[f"bcw weight w1 = {int(j['w1'])}"] += 1
            n["negative w1"] += int(j["weight_flag"] and j["w1"] < 0)
            n["explicit weights, P-typed slice, bi"] += int(sl == 2 and j["weight_flag"] and j["denom"] == 6)
            n["explicit weights, B-typed slice, bi"] += int(sl == 1 and j["weight_flag"] and j["denom"] == 6)
            n["dmvr_flag unit in the weighted B slice: unweighted"] += int(sl == 1 and pu["dmvr_flag"] and not j["weight_flag"])
            n["dmvr_flag unit in the weighted P slice: weighted"] += int(sl == 2 and pu["dmvr_flag"] and j["weight_flag"] and not r[4])
        else:
            n["explicit weights, P-typed slice, uni"] += int(sl == 2 and j["weight_flag"])
            n["explicit weights, B-typed slice, uni"] += int(sl == 1 and j["weight_flag"])
        if not j["dmvr"]:
            continue
        # DMVR: the refinement from the reference's table, the SAD from the oracle's record
        m0, m1 = pic.mvf[y >> 2, x >> 2], dmvr[y >> 2, x >> 2]
        assert np.array_equal(m1["mv"].reshape(-1), r[:4]), f"{pic.name}: job {i}: tab_dmvr_mvf and the oracle's record disagree"
        dx, dy = (int(v) for v in (m1["mv"][0] - m0["mv"][0]))
        assert (m1["mv"][1] - m0["mv"][1]).tolist() == [-dx, -dy]
        searched, min_sad = int(r[6]), int(r[5])
        if not searched:
            assert (dx, dy) == (0, 0) and min_sad < w * h
            n["DMVR ended early (min_sad < w * h)"] += 1
        elif max(abs(dx), abs(dy)) == 32:
            n["DMVR searched, minimum on the border of the 5x5 array"] += 1
        elif dx % 16 or dy % 16:
            n["DMVR searched, interior minimum, non-zero parametric step"] += 1
        if j["bdof"]:
            n["sb_bdof_flag cleared by min_sad < 2 * w * h" if not r[4] else "sb_bdof_flag kept after DMVR"] += 1
            assert bool(r[4]) == (min_sad >= 2 * w * h)
        for l in range(2):
            moved = (int(m1["mv"][l][0]) >> 4, int(m1["mv"][l][1]) >> 4) != (int(m0["mv"][l][0]) >> 4, int(m0["mv"][l][1]) >> 4)
            x_sb, y_sb = x + (int(m0["mv"][l][0]) >> 4), y + (int(m0["mv"][l][1]) >> 4)
            inside = x_sb - 3 >= 8 and y_sb - 3 >= 8 and x_sb + w + 4 <= W - 8 and y_sb + h + 4 <= H - 8
            n["refined block reads beyond the unrefined window, away from every picture edge"] += int(moved and inside)


def _affine_premises(pic, out, n, ph, shapes):
    jl, jc = out.aff_jl, out.aff_jc
    for cu in pic.aff:
        shapes.add((int(cu["cb_width"]), int(cu["cb_height"]), "affine"))
        pf = int(pic.mvf[int(cu["y0"]) >> 2, int(cu["x0"]) >> 2]["pred_flag"])
        n[f"affine {('L0', 'L1', 'bi')[pf - 1]}, cb_prof_flag {int(cu['prof_flags']) & pf}"] += 1
        n[f"affine unit in a slice with LMCS {'on' if pic.slices[int(cu['slice'])].lmcs_used else 'off'}"] += 1
    for j in jl:
        pf = int(j["pred_flag"])
        for l in range(2):
            if pf & (1 << l):
                _phases(ph, pic.idc, pic.hs, pic.vs, False, int(j["mv"][2 * l]), int(j["mv"][2 * l + 1]))
        if pf == 3 and j["weight_flag"]:
            n[f"affine bcw weight w1 = {int(j['w1'])}" if j["denom"] == 2 else "affine explicit weights, bi"] += 1
        n["affine explicit weights, uni"] += int(pf != 3 and j["weight_flag"])
    for j in jc:
        for l in range(2):
            if int(j["pred_flag"]) & (1 << l):
                _phases(ph, pic.idc, pic.hs, pic.vs, True, int(j["mv"][2 * l]), int(j["mv"][2 * l + 1]), luma=False)
    # derive_affine_mvc: sums that the rounding treats differently from a shift or a truncation
    if pic.chroma and (pic.hs or pic.vs):
        for cu in pic.aff:
            blk = pic.mvf[int(cu["y0"]) >> 2:(int(cu["y0"]) + int(cu["cb_height"])) >> 2, int(cu["x0"]) >> 2:(int(cu["x0"]) + int(cu["cb_width"])) >> 2]["mv"].astype(np.int64)
            s = blk[::1 << pic.vs, ::1 << pic.hs] + blk[pic.vs::1 << pic.vs, pic.hs::1 << pic.hs]
            n["derive_affine_mvc: odd negative sum"] += int(np.count_nonzero((s < 0) & (s & 1 == 1)))
            n["derive_affine_mvc: odd positive sum"] += int(np.count_nonzero((s > 0) & (s & 1 == 1)))


def _gpm_premises(pic, n, ph, shapes, partitions):
    t = ic.GPM_TABLES
    for cu in pic.gpm:
        shapes.add((int(cu["cb_width"]), int(cu["cb_height"]), "gpm"))
        part = int(cu["partition_idx"])
        partitions.add(part)
        n[f"GPM mirror type {int(t['ff_vvc_gpm_angle_to_mirror'][int(t['ff_vvc_gpm_angle_idx'][part])])}"] += 1
        mvs = cu["gpm_mv"].view(ic.ifc.MVF_DT)
        lists = [int(m["pred_flag"]) - 1 for m in mvs]
        n[f"GPM parts from L{lists[0]}, L{lists[1]}"] += 1
        sl = pic.slices[int(cu["slice"])]
        n["GPM unit in a slice with explicit weighting"] += int(sl.weighted_pred or sl.weighted_bipred)
        n[f"GPM unit in a slice with LMCS {'on' if sl.lmcs_used else 'off'}"] += 1
        for m, l in zip(mvs, lists):
            _phases(ph, pic.idc, pic.hs, pic.vs, True, int(m["mv"][l][0]), int(m["mv"][l][1]))


REGULAR_PREMISES = (
    ["hpel_if_idx 0", "hpel_if_idx 1", "BDOF alone", "DMVR alone", "DMVR and BDOF", "sub-block merge unit, 8x8 sub-blocks",
     "regular unit in a slice with LMCS on", "regular unit in a slice with LMCS off", "motion wholly outside the picture"] +
    [f"motion leaves the picture: {s}" for s in ("top", "bottom", "left", "right", "topleft", "topright", "bottomleft", "bottomright")] +
    [f"bcw weight w1 = {w}" for w in ic.BCW_W1[1:]] +
    ["negative w1", "explicit weights, P-typed slice, bi", "explicit weights, B-typed slice, bi", "explicit weights, P-typed slice, uni",
     "explicit weights, B-typed slice, uni", "dmvr_flag unit in the weighted B slice: unweighted", "dmvr_flag unit in the weighted P slice: weighted",
     "DMVR ended early (min_sad < w * h)", "DMVR searched, minimum on the border of the 5x5 array", "DMVR searched, interior minimum, non-zero parametric step",
     "sb_bdof_flag cleared by min_sad < 2 * w * h", "sb_bdof_flag kept after DMVR",
     "refined block reads beyond the unrefined window, away from every picture edge"])
AFFINE_PREMISES = (
    [f"affine {d}, cb_prof_flag {f}" for d, fl in (("L0", (0, 1)), ("L1", (0, 2)), ("bi", (0, 1, 2, 3))) for f in fl] +
    [f"affine bcw weight w1 = {w}" for w in ic.BCW_W1[1:]] +
    ["affine explicit weights, bi", "affine explicit weights, uni", "affine unit in a slice with LMCS on", "affine unit in a slice with LMCS off",
     "derive_affine_mvc: odd negative sum", "derive_affine_mvc: odd positive sum"])
GPM_PREMISES = ([f"GPM mirror type {m}" for m in range(3)] + [f"GPM parts from L{a}, L{b}" for a in (0, 1) for b in (0, 1)] +
                ["GPM unit in a slice with explicit weighting", "GPM unit in a slice with LMCS on", "GPM unit in a slice with LMCS off"])
CIIP_PREMISES = [f"CIIP intra weight {w}" for w in (1, 2, 3)] + ["CIIP unit 4 wide at 4:2:0 or 4:2:2: chroma 2 wide, not blended", "CIIP luma through the forward map",
                                                                  "CIIP bcw_idx ignored", "CIIP explicit weights"]


def test_premises_of_the_listed_pictures(orc, ref, golden):
    t0, n, ph, shapes, partitions, conf = time.time(), Counter(), defaultdict(set), set(), set(), []
    for name in ic.REGULAR + ic.AFFINE + ic.GPM + [ic.MIXED]:
        pic = ic.picture(name)
        assert pic.width <= 256 and pic.height <= 192
        conf.append((pic.kinds, pic.bd, pic.idc, pic.ctb_log2, pic.width % (1 << pic.ctb_log2) != 0 and pic.height % (1 << pic.ctb_log2) != 0))
        out = ic.run_picture(orc, "orc", pic)
        if ref is not None:
            dmvr = ic.run_picture(ref, "ref", pic).dmvr
        else:
            assert ic.host_digests(orc, "orc", name) == golden[name], f"{name}: the oracle does not reproduce the reference's digests"
            dmvr = out.dmvr
        for c, p in enumerate(out.planes):
            outside = ~pic.covered[::1 << (pic.vs if c else 0), ::1 << (pic.hs if c else 0)]
            assert outside.any() and (p[outside] == pic.sentinel).all() and (p[~outside] != pic.sentinel).mean() > 0.9, f"{name}: component {c}"
        # units in CTU order, CTU-aligned slices
        for rec in (pic.pus, pic.aff, pic.gpm):
            rs = [(int(u["y0"]) >> pic.ctb_log2) * pic.ncx + (int(u["x0"]) >> pic.ctb_log2) for u in rec]
            assert rs == sorted(rs) and all(int(u["slice"]) == pic.ctu_slice[r] for u, r in zip(rec, rs))
        if "R" in pic.kinds:
            _regular_premises(pic, out, dmvr, n, ph, shapes)
        if "A" in pic.kinds:
            _affine_premises(pic, out, n, ph, shapes)
        if "G" in pic.kinds:
            _gpm_premises(pic, n, ph, shapes, partitions)
    for name in ic.CIIP:
        cp = ic.ciip_picture(name)
        p = cp.p
        assert p.width <= 256 and p.height <= 192
        assert all(int(cu["slice"]) == int(p.slice_idx[(int(cu["y0"]) >> p.ctb_log2) * p.ncx + (int(cu["x0"]) >> p.ctb_log2)]) for cu in p.cus), f"{name}: slices inside a CTU"
        conf.append(("I", cp.bd, p.idc, p.ctb_log2, False))
        if ref is not None:
            weights = ic.run_ciip(ref, "ref", cp).weights
        else:
            assert ic.host_digests(orc, "orc", name) == golden[name], f"{name}: the oracle does not reproduce the reference's digests"
            weights = ic.run_ciip(orc, "orc", cp).weights
        for u, cu in enumerate(p.cus):
            n[f"CIIP intra weight {int(weights[u, 0])}"] += 1
            n["CIIP unit 4 wide at 4:2:0 or 4:2:2: chroma 2 wide, not blended"] += int(p.chroma and p.hs and cu["cb_width"] == 4 and weights[u, 1] == 0)
            m = p.mvf[int(cu["y0"]) >> 2, int(cu["x0"]) >> 2]
            n["CIIP luma through the forward map"] += int(p.slices[int(cu["slice"])].lmcs_used)
            n["CIIP bcw_idx ignored"] += int(m["pred_flag"] == 3 and m["bcw_idx"] > 0)
            n["CIIP explicit weights"] += int(p.slices[int(cu["slice"])].weighted_bipred and m["bcw_idx"] == 0)
    premises = REGULAR_PREMISES + AFFINE_PREMISES + GPM_PREMISES + CIIP_PREMISES
    for key in premises:
        print(f"{key}: {n[key]}")
    missing = [key for key in premises if n[key] <= 0]
    assert not missing, f"premises that hold nowhere in the list: {missing}"
    assert set(n) <= set(premises), sorted(set(n) - set(premises))
    # every interpolation phase that the format can reach (the chroma phase of an unshifted direction is twice the luma phase: even values)
    for idc in (0, 1, 2, 3):
        hs, vs = ic.FMT[idc]
        assert ph[(idc, "luma x")] == set(range(16)) and ph[(idc, "luma y")] == set(range(16)), f"luma phases at chroma_format_idc {idc}"
        if idc:
            assert ph[(idc, "chroma x")] == set(range(0, 32, 1 if hs else 2)), (idc, sorted(ph[(idc, "chroma x")]))
            assert ph[(idc, "chroma y")] == set(range(0, 32, 1 if vs else 2)), (idc, sorted(ph[(idc, "chroma y")]))
    # unit sizes
    assert {(4, 8, "uni"), (8, 4, "uni"), (4, 16, "uni"), (16, 4, "uni")} <= shapes
    for wh in ((8, 8), (16, 16), (32, 32), (64, 64), (128, 128), (128, 64)):
        assert (*wh, "plain") in shapes and (wh == (8, 8) or (*wh, "flags") in shapes), f"no bi-predicted {wh} unit both with and without DMVR / BDOF"
    assert (128, 128, "affine") in shapes
    assert sorted((w, h) for w, h, k in shapes if k == "gpm") == ic.GPM_SHAPES and partitions == set(range(64))
    # formats, depths, CTU sizes per driver kind; two regular pictures that are no multiple of the CTU either way
    for kind in "RAGI":
        mine = [c for c in conf if kind in c[0]]
        assert {c[1] for c in mine} == {8, 10, 12} and {c[3] for c in mine} == {5, 6, 7}, kind
        assert {c[2] for c in mine} >= ({1, 2, 3} if kind == "G" else {0, 1, 2, 3}), kind
    assert sum(c[4] for c in conf if c[0] == "R") >= 2
    print(f"{len(premises)} premises hold, counted in {time.time() - t0:.1f} s")

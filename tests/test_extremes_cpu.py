"""CPU: the full-scale worst-case pictures of tests/extreme_cases.py.

* Premises (everywhere): what the pictures must reach, asserted from numpy restatements of the rules and from the oracle's outputs, never
  from the device.
* Live (where oracle/_ref/libvvcref.so is built, skipped elsewhere): oracle == reference on every picture, planes compared whole.
* Digests (everywhere): the oracle reproduces tests/golden/ref_extremes.json, and the generators still hash to the recorded inputs."""
import os
import sys
from collections import Counter

from types import SimpleNamespace

import numpy as np
import pytest

import ciip_frame_cases as cc
import extreme_cases as xc
import ref_inter_cases as ic
import ref_lib
import ref_pass_cases as pc


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


@pytest.fixture(scope="module")
def ref():
    return ref_lib.load()


@pytest.fixture(scope="module")
def golden():
    return xc.load_golden()


def _need(ref):
    if ref is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")


# ---------------------------------------------------------------------------------------------------------------- live

@pytest.mark.parametrize("name", xc.SAO + xc.ALF + xc.ALF_CC)
def test_live_filters_equal_the_reference(ref, orc, name):
    _need(ref)
    fp = xc.filter_picture(name)
    for s in fp.stages:
        lines = pc.plane_differences(name, s, pc.run_filter(ref, "ref", fp, s), pc.run_filter(orc, "orc", fp, s))
        assert not lines, "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- digests

@pytest.mark.parametrize("name", xc.picture_names())
def test_oracle_reproduces_reference_digests(golden, orc, ref, name):
    assert name in golden, f"{name} is not in ref_extremes.json: regenerate it (tests/golden/README.md)"
    got = xc.host_digests(orc, "orc", name)
    assert got["inputs"] == golden[name]["inputs"], f"generator drifted: the inputs of {name} no longer hash to the recorded digest"
    assert set(got) == set(golden[name]), f"{name}: keys differ: {sorted(set(got) ^ set(golden[name]))}"
    bad = sorted(k for k in got if got[k] != golden[name][k])
    assert not bad, f"{name}: the oracle's {bad} do not hash to the reference's digests" + ("" if ref is None else "; test_live_* names the sample")


def test_no_picture_left_out(golden):
    assert list(golden) == xc.picture_names()


def test_fixture_is_fresh(ref, orc):
    _need(ref)
    sys.path.insert(0, os.path.join(ref_lib.ROOT, "tools"))
    import gen_golden
    with open(xc.GOLDEN_PATH) as f:
        assert f.read() == gen_golden.dumps_passes(gen_golden.generate_extremes(ref)), "tests/golden/ref_extremes.json is stale: python tools/gen_golden.py"


# ---------------------------------------------------------------------------------------------------------------- premises: SAO

_SAO_NB = (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((1, -1), (-1, 1)))          # (dx, dy) of the two neighbours per edge class
_SAO_CAT = (1, 2, 0, 3, 4)                                                                         # edge index 0..4 -> offset_val index


def _sao_premises(fp, out, n):
    """Band CTBs whole, edge CTBs away from their own border (where the restore rules of slices, tiles and the picture do not reach): the
    oracle's output is clip(sample + offset) by h2656_sao_template.c's rules restated here; counts what clipped."""
    t, bd = fp.t, fp.bd
    top = (1 << bd) - 1
    ctb = 1 << t.ctb_log2
    sao = np.frombuffer(fp.sao.tobytes(), dtype=np.dtype([("off", "<i2", (3, 5)), ("ty", "u1", (3,)), ("pos", "u1", (3,)), ("eo", "u1", (3,)), ("pad", "u1")]))
    for c in range(fp.n_comp):
        hs, vs = (t.hs, t.vs) if c else (0, 0)
        src, got = fp.planes[c].astype(np.int64), out[c].astype(np.int64)
        ph, pw = src.shape
        for rs in range(t.cw * t.ch):
            x0, y0 = (rs % t.cw) * ctb >> hs, (rs // t.cw) * ctb >> vs
            w, h = min(ctb >> hs, pw - x0), min(ctb >> vs, ph - y0)
            off, ty, pos, eo = sao["off"][rs, c].astype(np.int64), int(sao["ty"][rs, c]), int(sao["pos"][rs, c]), int(sao["eo"][rs, c])
            assert set(np.abs(off[1:]).tolist()) == {(1 << (bd - 5)) - 1}
            if ty == 1:
                s = src[y0:y0 + h, x0:x0 + w]
                k = ((s >> (bd - 5)) - pos) & 31
                v = s + np.where(k < 4, off[np.minimum(k, 3) + 1], 0)
                key = "band"
                n[(bd, "band position", pos, tuple(np.sign(off[1:]).tolist()))] += 1
                want, have = np.clip(v, 0, top), got[y0:y0 + h, x0:x0 + w]
            else:
                assert ty == 2
                if w < 3 or h < 3:
                    continue
                s = src[y0 + 1:y0 + h - 1, x0 + 1:x0 + w - 1]
                (ax, ay), (bx, by) = _SAO_NB[eo]
                a = src[y0 + 1 + ay:y0 + h - 1 + ay, x0 + 1 + ax:x0 + w - 1 + ax]
                b = src[y0 + 1 + by:y0 + h - 1 + by, x0 + 1 + bx:x0 + w - 1 + bx]
                v = s + off[np.array(_SAO_CAT)[2 + np.sign(s - a) + np.sign(s - b)]]
                key = "edge"
                n[(bd, "edge class", eo, tuple(np.sign(off[1:]).tolist()))] += 1
                want, have = np.clip(v, 0, top), got[y0 + 1:y0 + h - 1, x0 + 1:x0 + w - 1]
            assert np.array_equal(want, have), f"{fp.name}: component {c}, CTB {rs} ({key}): the oracle's output is not clip(sample + offset)"
            n[(bd, key, "clipped at 0")] += int(np.count_nonzero(v < 0))
            n[(bd, key, "clipped at the maximum")] += int(np.count_nonzero(v > top))
            # where the saturating 16-bit add of the packed kernel would matter: none can overflow int16, the clip is to the sample range
            assert int(v.min()) >= -(1 << 15) and int(v.max()) < (1 << 15)


def test_sao_premises(orc):
    n = Counter()
    for name in xc.SAO:
        fp = xc.filter_picture(name)
        before = Counter(n)
        _sao_premises(fp, pc.run_filter(orc, "orc", fp, "sao"), n)
        # every picture clips at both ends, in band and in edge mode
        for key in ("band", "edge"):
            for end in ("clipped at 0", "clipped at the maximum"):
                assert n[(fp.bd, key, end)] > before[(fp.bd, key, end)], f"{name}: no {key} sample {end}"
    want = [(bd, key, end) for bd in (8, 10, 12) for key in ("band", "edge") for end in ("clipped at 0", "clipped at the maximum")]
    want += [(bd, "band position", pos, signs) for bd in (8, 10, 12) for pos in range(32) for signs in ((1, 1, 1, 1), (-1, -1, -1, -1))]
    want += [(bd, "edge class", eo, signs) for bd in (8, 10, 12) for eo in range(4) for signs in xc.SAO_SIGNS]
    missing = [k for k in want if n[k] <= 0]
    assert not missing, f"SAO premises that hold nowhere: {missing}"
    for bd in (8, 10, 12):
        print(bd, {k[1:]: v for k, v in n.items() if k[0] == bd and len(k) == 3})


# ---------------------------------------------------------------------------------------------------------------- premises: ALF

def _alf_forms(fp, k, n, cens):
    """Counts, by the rule of the CTB kernel restated here (alf.hip, "the clamp-free form carries the centre weight ..."): a CTB is clamp-free
    when every (class, tap) of its filter set has clip index 0 or coefficient 0 — every fixed set, and the APS set whose clip indices are
    0; a block's kind is 1 in the block row that ends at the virtual boundary ctb - 4, 2 in the one that starts there, 0 elsewhere.  Kind 3
    (a block that straddles the boundary or lies closer than three rows to it without touching it) cannot occur in the stage driver: the
    boundary and the blocks are both on the 4-grid."""
    t = fp.t
    ctb, vb = 1 << t.ctb_log2, (1 << t.ctb_log2) - 4
    alf = fp.alf.reshape(-1, 8)
    for rs in range(t.cw * t.ch):
        if not alf[rs, 0]:
            continue
        set_idx = int(alf[rs, 3])
        x0, y0 = (rs % t.cw) * ctb, (rs // t.cw) * ctb
        w, h = min(ctb, t.width - x0), min(ctb, t.height - y0)
        if set_idx < 16:
            noclip, coeff = True, None
        else:
            coeff, clip_idx = fp.aps[set_idx - 16].astype(np.int64), fp.aps[2 + set_idx - 16]
            noclip = not np.any((clip_idx != 0) & (coeff != 0))
        for yb in range(0, h, 4):
            near = min(abs(vb - 1 - yb) if yb < vb else yb - vb, abs(vb - 1 - yb - 3) if yb + 3 < vb else yb + 3 - vb) < 3 or (yb < vb <= yb + 3)
            kind = 0 if not near else 1 if yb + 4 == vb else 2 if yb == vb else 3
            assert kind < 3
            n[("clamp-free" if noclip else "clamped", kind)] += w // 4
            if coeff is not None:
                for bx in range(x0 // 4, (x0 + w) // 4):
                    cen = -2 * int(coeff[k.cls[(y0 + yb) // 4, bx]].sum())
                    assert -32768 <= cen and cen + 1024 <= 32767                # the 16-bit operand of the clamp-free form
                    cens[(noclip, cen)] += 1


def test_alf_premises(orc):
    n, cens, reached = Counter(), Counter(), {}
    seen_cls, seen_tr = set(), set()
    for name in xc.ALF:
        fp = xc.filter_picture(name)
        k = xc.alf_classify(fp.planes[0], fp.bd, fp.t.ctb_log2)
        _alf_forms(fp, k, n, cens)
        seen_cls |= set(k.cls[k.inner].ravel().tolist())
        seen_tr |= set(k.tr[k.inner].ravel().tolist())
        top = (1 << fp.bd) - 1
        # four cells side by side, two samples each, |2s - a - b| <= 2 * top: the largest 16-bit half the CTB kernel forms
        assert int(k.rowmax.max()) <= 16 * top
        for d, label in enumerate("V H D0 D1".split()):
            if int(k.rowmax[k.inner][:, d].max()) == 16 * top:
                reached.setdefault((fp.bd, label), name)
        out = pc.run_filter(orc, "orc", fp, "alf")
        # a sample that the filter moved onto an end of the range (the patterns hold nothing but the two ends, so it crossed the whole range)
        ends = Counter()
        for c in range(3):
            changed = out[c] != fp.planes[c]
            ends[0] += int(np.count_nonzero(changed & (out[c] == 0)))
            ends[top] += int(np.count_nonzero(changed & (out[c] == top)))
            assert np.any(changed), f"{name}: component {c} unchanged by ALF"
        assert ends[0] and ends[top], f"{name}: ALF clipped at neither end: {dict(ends)}"
    # 12 bit: 16 * 4095 = 65 520 of 65 535 in every direction
    for label in "V H D0 D1".split():
        assert (12, label) in reached, f"no 12-bit picture drives the horizontal cell sum of {label} to 65 520"
    # what full-scale content can reach: the activity (sum of V and H, scaled) is 0 on flat content and saturates at 4 on every pattern, so
    # the class is 0 or 4 + 5 * direction; every transpose index occurs
    assert seen_cls == set(xc.ALF_REACHED), sorted(seen_cls)
    assert seen_tr == {0, 1, 2, 3}, sorted(seen_tr)
    missing = [(form, kind) for form in ("clamp-free", "clamped") for kind in (0, 1, 2) if n[(form, kind)] <= 0]
    assert not missing, f"ALF forms / boundary kinds that ran nowhere: {missing}"
    # the centre weight -2 * sum(f) at both ends of what the coefficient range allows, in both forms
    for noclip in (True, False):
        assert cens[(noclip, -2 * 12 * xc.ALF_COEFF_MAX)] > 0 and cens[(noclip, -2 * 12 * xc.ALF_COEFF_MIN)] > 0, sorted(cens)
    print(dict(n), reached)


def test_alf_classification_restated_equals_the_oracle(orc):
    """The numpy classification the premises use against orc_alf_classify, CTB by CTB, on every CTB away from the picture's border."""
    checked = 0
    for name in xc.ALF:
        fp = xc.filter_picture(name)
        t, bd, luma = fp.t, fp.bd, fp.planes[0]
        k = xc.alf_classify(luma, bd, t.ctb_log2)
        ctb = 1 << t.ctb_log2
        for rs in range(t.cw * t.ch):
            x0, y0 = (rs % t.cw) * ctb, (rs // t.cw) * ctb
            w, h = min(ctb, t.width - x0), min(ctb, t.height - y0)
            if x0 < 4 or y0 < 4 or x0 + w + 4 > t.width or y0 + h + 4 > t.height:
                continue
            nb = (w // 4) * (h // 4)
            cls, tr, tmp = np.zeros(nb, np.int32), np.zeros(nb, np.int32), np.zeros((h + 8) * (w + 8) * 4, np.int32)
            orc.orc_alf_classify(bd, cls.ctypes.data, tr.ctypes.data, luma.ctypes.data + y0 * luma.strides[0] + x0 * luma.itemsize, luma.strides[0], w, h,
                                 ctb - 4, tmp.ctypes.data)
            sel = (slice(y0 // 4, (y0 + h) // 4), slice(x0 // 4, (x0 + w) // 4))
            assert np.array_equal(k.cls[sel].ravel(), cls) and np.array_equal(k.tr[sel].ravel(), tr), f"{name}: CTB {rs}"
            checked += 1
    assert checked >= 12, checked


# ---------------------------------------------------------------------------------------------------------------- inter pictures

INTER = xc.REGULAR + xc.AFFINE + xc.GPM


@pytest.mark.parametrize("name", INTER)
def test_live_inter_equals_the_reference(ref, orc, name):
    _need(ref)
    pic, _ = xc.inter_picture(name)
    want, got = ic.run_picture(ref, "ref", pic), ic.run_picture(orc, "orc", pic)
    lines = ic.plane_differences(pic, want.planes, got.planes)
    if "R" in pic.kinds:
        lines += ic.dmvr_differences(pic, want.dmvr, got.dmvr)
    assert not lines, "\n".join(lines)


def _marked_intermediates(pic, units, u):
    """Per list and component of a unit on sign-matched tiles: [(list, component, bounds, first-pass values, value)] at every marked sample, in
    int64 from the reference planes."""
    out = []
    for l, (fx, fy, inv, content) in u["lists"].items():
        if content != ("tile", "hv"):
            continue
        for c in range(3 if pic.chroma else 1):
            hrow, vrow, px_, py_ = units.rows(u, l, c)
            hs, vs = (pic.hs, pic.vs) if c else (0, 0)
            b = xc.pass_bounds(hrow, vrow, px_, py_, pic.bd)
            for (x, y) in xc.marked(u):
                first, val = xc.intermediate(pic.refs[l][inv][c], x >> hs, y >> vs, hrow, vrow, px_, py_, pic.bd)
                if px_ and py_:
                    first = first[vrow != 0]          # a row under a zero tap (the 6-tap rows' ends) is read, not used
                out.append((l, c, inv, b, first, val))
    return out


@pytest.mark.parametrize("name", [n for n in INTER if n not in xc.VARYING])
def test_marked_samples_reach_the_analytic_bounds(name):
    """On the tile the marked samples' intermediate is the largest the phase pair allows, on the inverse the smallest, and after the first
    pass every row the sample reads sits on one of the two first-pass bounds."""
    pic, units = xc.inter_picture(name)
    n = 0
    for u in units.read:
        for (l, c, inv, b, first, val) in _marked_intermediates(pic, units, u):
            assert val == b["second"][0 if inv else 1], f"{name}: unit at ({u['x']}, {u['y']}) list {l} component {c}: {val} is not the bound {b['second']}"
            assert set(first.tolist()) <= set(int(v) for v in b["first"]), (name, u["x"], u["y"], l, c, first, b["first"])
            n += 1
    assert n >= 40, n


def test_phase_pairs_all_walked():
    """Every luma phase pair of {0, 8, 7, 9}^2 on the tile and on the inverse at every bit depth in the regular pictures; the half-sample
    alternative filter, every bcw_idx, both LMCS settings and uni- and bi-predicted units in every weighting regime."""
    seen, kinds = set(), set()
    assert xc.luma_phases() == (0, 8, 7, 9)
    for name in xc.REGULAR:
        pic, units = xc.inter_picture(name)
        for u in units.read:
            for l, (fx, fy, inv, content) in u["lists"].items():
                if content == ("tile", "hv"):
                    seen.add((pic.bd, fx, fy, inv))
            sl = pic.slices[u["slice"]]
            kinds.add((pic.bd, len(u["lists"]), bool(sl.weighted_pred or sl.weighted_bipred), bool(sl.lmcs_used)))
            kinds.add((pic.bd, "bcw", u["bcw"]))
            kinds.add((pic.bd, "hpel", u["hpel"]))
            kinds.add((pic.bd, "dmvr/bdof", u["dmvr"], u["bdof"]))
    for bd in (8, 10, 12):
        missing = [(fx, fy, inv) for fx in (0, 8, 7, 9) for fy in (0, 8, 7, 9) for inv in (0, 1) if (bd, fx, fy, inv) not in seen]
        assert not missing, (bd, missing)
        want = [(bd, n, w, lm) for n in (1, 2) for (w, lm) in ((False, True), (False, False), (True, False))] + [(bd, 1, True, True)]
        want += [(bd, "bcw", k) for k in range(5)] + [(bd, "hpel", k) for k in (0, 1)] + [(bd, "dmvr/bdof", d, b) for d in (0, 1) for b in (0, 1)]
        assert not [k for k in want if k not in kinds], (bd, [k for k in want if k not in kinds])


def test_twelve_bit_sums_leave_int16():
    """What the packed kernels must survive at 12 bit, from the int64 intermediates of the marked samples of XR2 / XR5 / XR6 / XR7:
    * one prediction after two passes exceeds a signed half: with the half-sample filter in both directions the sign-matched tile gives
      (88 * 22522 + 24 * 6143) >> 6 = 33271 > 32767 (the reference stores it in int16_t, where it wraps; oracle and device are held to that);
      no phase pair reaches below -32768 with one prediction (the smallest is -16893);
    * the sum s0 + s1 of a bi-predicted unit is above 32767 on tiles and below -32768 on inverses: both ends are reachable."""
    hi = lo = 0
    one_hi, one_lo = 0, 0
    for name in ("XR2", "XR5", "XR6", "XR7"):
        pic, units = xc.inter_picture(name)
        assert pic.bd == 12
        for u in units.read:
            vals = {}
            for (l, c, inv, b, first, val) in _marked_intermediates(pic, units, u):
                if c == 0:
                    vals.setdefault(l, []).append(int(val))
                    one_hi, one_lo = max(one_hi, int(val)), min(one_lo, int(val))
            if len(vals) == 2 and len(u["lists"]) == 2:
                s = [a + b_ for a, b_ in zip(vals[0], vals[1])]
                hi, lo = max(hi, max(s)), min(lo, min(s))
    luma, _ = xc.filter_rows()
    b = xc.pass_bounds(luma[0][8], luma[0][8], 8, 8, 12)
    assert (int(b["first"][0]), int(b["first"][1]), int(b["second"][0]), int(b["second"][1])) == (-6143, 22522, -16893, 33271)
    assert one_hi == 33271 and one_lo == -16893, (one_hi, one_lo)
    assert hi > 32767 and lo < -32768, (hi, lo)
    print(f"12 bit: one prediction {one_lo} .. {one_hi}, s0 + s1 {lo} .. {hi}")


def _pre_clip(bd, vals, wt):
    """The value before clip_px of one luma sample from its lists' int64 intermediates `vals` {list: value} and derive_weight's result `wt` =
    (weight_flag, denom, w0, w1, o0, o1): put_uni / put_uni_w round the int; avg / w_avg read what put stored in int16_t."""
    flag, denom, w0, w1, o0, o1 = (int(v) for v in wt)
    if len(vals) == 1:
        (v,) = (int(x) for x in vals.values())
        if not flag:
            return (v + (1 << (13 - bd))) >> (14 - bd)
        sh = denom + 14 - bd
        return ((v * w0 + (1 << (sh - 1))) >> sh) + o0 * (1 << (bd - 8))
    s0, s1 = int(_i16(vals[0])), int(_i16(vals[1]))
    if not flag:
        return (s0 + s1 + (1 << (14 - bd))) >> (15 - bd)
    sh = denom + 15 - bd
    return (s0 * w0 + s1 * w1 + ((((o0 + o1) << (bd - 8)) + 1) << (sh - 1))) >> sh


def _luma_values(pic, units, u):
    """{marked position: {list: int64 intermediate}} of a unit whose lists all read tiles."""
    if any(v[3] != ("tile", "hv") for v in u["lists"].values()):
        return {}
    out = {}
    for pos in xc.marked(u):
        out[pos] = {}
    for (l, c, inv, b, first, val), pos in zip([m for m in _marked_intermediates(pic, units, u) if m[1] == 0], xc.marked(u) * len(u["lists"])):
        out[pos][l] = val
    return out


def _gpm_weight(cu, x, y):
    """The blend weight of pred_gpm_blk's mask at sample (x, y) of a 16x16 unit (vvc_inter.c:466-497)."""
    part = int(cu["partition_idx"])
    angle = int(ic.GPM_TABLES["ff_vvc_gpm_angle_idx"][part])
    mirror = int(ic.GPM_TABLES["ff_vvc_gpm_angle_to_mirror"][angle])
    off_x, off_y = (int(ic.GPM_TABLES[f"ff_vvc_gpm_weights_offset_{k}"][part, 1, 1]) for k in "xy")
    mask = ic.GPM_MASKS[int(ic.GPM_TABLES["ff_vvc_gpm_angle_to_weights_idx"][angle])].reshape(112, 112)
    return int(mask[off_y + y, 111 - off_x - x] if mirror == 1 else mask[111 - off_y - y, off_x + x] if mirror == 2 else mask[off_y + y, off_x + x])


# pictures that cannot clip at both ends, and why
ONE_END = {"XR7": "one 128x128 bi-predicted unit whose two lists both read the inverse tile: every marked sample lies below 0"}


@pytest.mark.parametrize("name", INTER + xc.CIIP)
def test_every_inter_picture_clips_at_both_ends(orc, name):
    """Per picture: the value before clip_px of the marked luma samples, restated in int64 from the intermediates and derive_weight's result
    for uni, bi, bcw and explicitly weighted units (affine: the units without PROF; GPM: put_gpm with the mask's weight), is below 0
    somewhere and above the maximum somewhere, and the oracle's sample is its clip (through the forward map where the slice uses LMCS).
    Every component's output also holds both ends inside the units."""
    ciip = name in xc.CIIP
    if ciip:
        cp, units = xc.ciip_picture(name)
        p = cp.p
        pic = SimpleNamespace(refs=cp.refs, chroma=True, hs=p.hs, vs=p.vs, bd=cp.bd, slices=p.slices, mvf=p.mvf, lut=cp.lut)
        run = ic.run_ciip(orc, "orc", cp)
    else:
        pic, units = xc.inter_picture(name)
        out = ic.run_picture(orc, "orc", pic)
        for c, plane in enumerate(out.planes):
            hs, vs = (pic.hs, pic.vs) if c else (0, 0)
            cov = pic.covered[::1 << vs, ::1 << hs]
            assert np.any(cov & (plane == 0)) and np.any(cov & (plane == (1 << pic.bd) - 1)), f"{name}: component {c} does not reach both ends"
    bd, top = pic.bd, (1 << pic.bd) - 1
    over = under = checked = 0
    for k, u in enumerate(units.read):
        if u["dmvr"] or u["bdof"] or u["prof"]:
            continue
        m = pic.mvf[u["y"] // 4, u["x"] // 4]
        for (x, y), vals in _luma_values(pic, units, u).items():
            if name[1] == "G":
                w = _gpm_weight(pic.gpm[k], x - u["x"], y - u["y"])
                pre = (int(_i16(vals[0])) * w + int(_i16(vals[1])) * (8 - w) + (1 << (16 - bd))) >> (17 - bd)
            else:
                wt = cc.weights(pic.slices, u["slice"], m, 0) if ciip else pic.weights(u["slice"], m, 0)
                if len(vals) == 1 and not wt[0] and not any(u["lists"][l][0] or u["lists"][l][1] for l in vals):
                    continue                                    # put_uni at an integer position copies the sample
                pre = _pre_clip(bd, vals, wt)
            over, under = over + (pre > top), under + (pre < 0)
            want = min(top, max(0, pre))
            if pic.slices[u["slice"]].lmcs_used:
                want = int(pic.lut[want])
            if ciip:
                got = int(run.scratch[int(p.cus[k]["scratch_off"]) + (y - u["y"]) * u["w"] + (x - u["x"])])
            else:
                got = int(out.planes[0][y, x])
            assert got == want, (name, u["x"], u["y"], vals, pre, got, want)
            checked += 1
    print(name, "marked samples checked", checked, "above the maximum", over, "below 0", under)
    if name in xc.VARYING:          # no tiles: nothing is marked; the planes' both ends were asserted above
        assert checked == 0
        return
    assert checked > 0
    if name in ONE_END:
        assert under > 0 and over == 0, (name, over, under)
    else:
        assert over > 0 and under > 0, (name, over, under)


def test_dmvr_searched_on_extreme_units(orc):
    """The DMVR units on the zero / maximum pair, on checker1 against its inverse and on tiles: the search ran (no early exit) on at least one
    unit of each kind of content at each bit depth, by the oracle's records."""
    searched = Counter()
    for name in xc.REGULAR:
        pic, units = xc.inter_picture(name)
        out = ic.run_picture(orc, "orc", pic)
        for p, u in zip(pic.pus, units.read):
            if u["dmvr"]:
                rec = out.rec[int(p["first_job"])]
                searched[(pic.bd, u["lists"][0][3])] += int(rec[6])
    for bd in (8, 10, 12):
        for content in (("plain", "zero"), ("plain", "checker1"), ("tile", "h")):
            assert searched[(bd, content)] > 0, (bd, content, dict(searched))


def _i16(a):
    return ((a + 32768) % 65536) - 32768


def _bdof_unit(pic, u):
    """BDOF of one 16x16 unit restated from vvc_inter_template.c (bdof_fetch_samples, prof_grad_filter with its replicated ring, the 6x6
    windows of derive_bdof_vx_vy, apply_bdof_min_block) in int64 with the int16_t stores written out: ([(vx, vy)] per 4x4, the block)."""
    luma, _ = xc.filter_rows()
    bd, x0, y0, w, h = pic.bd, u["x"], u["y"], u["w"], u["h"]
    planes = []
    for l in range(2):
        fx, fy, inv, _content = u["lists"][l]
        p = np.pad(pic.refs[l][inv][0].astype(np.int64), 8, mode="edge")
        hrow, vrow = luma[u["hpel"]][fx], luma[u["hpel"]][fy]
        win = p[8 + y0 - 3:8 + y0 + h + 4, 8 + x0 - 3:8 + x0 + w + 4]
        if fx and fy:
            first = _i16(sum(hrow[k] * win[:, k:k + w] for k in range(8)) >> (bd - 8))
            val = sum(vrow[k] * first[k:k + h] for k in range(8)) >> 6
        elif fx:
            val = sum(hrow[k] * win[3:3 + h, k:k + w] for k in range(8)) >> (bd - 8)
        elif fy:
            val = sum(vrow[k] * win[k:k + h, 3:3 + w] for k in range(8)) >> (bd - 8)
        else:
            val = win[3:3 + h, 3:3 + w] << (14 - bd)
        a = np.zeros((h + 2, w + 2), np.int64)
        a[1:-1, 1:-1] = _i16(val)
        xo, yo = (fx >> 3) - 1, (fy >> 3) - 1                               # the ring: the nearest integer sample, scaled to 14 bits
        ring = p[8 + y0 + yo:8 + y0 + yo + h + 2, 8 + x0 + xo:8 + x0 + xo + w + 2] << (14 - bd)
        edge = np.ones(a.shape, bool)
        edge[1:-1, 1:-1] = False
        a[edge] = _i16(ring)[edge]
        planes.append(a)
    grads = []
    for a in planes:
        gh, gv = _i16((a[1:-1, 2:] >> 6) - (a[1:-1, :-2] >> 6)), _i16((a[2:, 1:-1] >> 6) - (a[:-2, 1:-1] >> 6))
        grads.append((np.pad(gh, 1, mode="edge"), np.pad(gv, 1, mode="edge")))
    s = [np.pad(a[1:-1, 1:-1], 1, mode="edge") for a in planes]            # pad_sample: the ring now repeats the block's own border
    sh = 15 - bd
    out, vs = np.zeros((h, w), np.int64), []
    for by in range(0, h, 4):
        for bx in range(0, w, 4):
            sl = (slice(by, by + 6), slice(bx, bx + 6))
            diff = (s[0][sl] >> 4) - (s[1][sl] >> 4)
            th, tv = (grads[0][0][sl] + grads[1][0][sl]) >> 1, (grads[0][1][sl] + grads[1][1][sl]) >> 1
            sgx2, sgy2, sgxgy = int(np.abs(th).sum()), int(np.abs(tv).sum()), int((np.sign(tv) * th).sum())
            sgxdi, sgydi = int((-np.sign(th) * diff).sum()), int((-np.sign(tv) * diff).sum())
            vx = max(-15, min(15, (sgxdi * 4) >> (sgx2.bit_length() - 1))) if sgx2 > 0 else 0
            vy = max(-15, min(15, ((sgydi * 4) - ((vx * sgxgy) >> 1)) >> (sgy2.bit_length() - 1))) if sgy2 > 0 else 0
            vs.append((vx, vy))
            c = (slice(by + 1, by + 5), slice(bx + 1, bx + 5))
            corr = vx * (grads[0][0][c] - grads[1][0][c]) + vy * (grads[0][1][c] - grads[1][1][c])
            out[by:by + 4, bx:bx + 4] = np.clip((s[0][c] + (1 << (sh - 1)) + s[1][c] + corr) >> sh, 0, (1 << bd) - 1)
    return vs, out


def test_bdof_refinements_reach_the_clip(orc):
    """The BDOF-only units (their motion is known without a search): the restatement reproduces the oracle's block, and vx and vy reach -15
    and +15 at every bit depth."""
    reached = {bd: set() for bd in (8, 10, 12)}
    for name in xc.REGULAR[:7]:
        pic, units = xc.inter_picture(name)
        out = ic.run_picture(orc, "orc", pic)
        for u in units.read:
            if not u["bdof"] or u["dmvr"]:
                continue
            vs, blk = _bdof_unit(pic, u)
            if pic.slices[u["slice"]].lmcs_used:
                blk = pic.lut.astype(np.int64)[blk]
            assert np.array_equal(out.planes[0][u["y"]:u["y"] + 16, u["x"]:u["x"] + 16], blk), f"{name}: BDOF unit at ({u['x']}, {u['y']}) restated wrongly"
            for vx, vy in vs:
                reached[pic.bd] |= {("vx", vx), ("vy", vy)}
    for bd, got in reached.items():
        assert {("vx", -15), ("vx", 15), ("vy", -15), ("vy", 15)} <= got, (bd, sorted(got))


# ---------------------------------------------------------------------------------------------------------------- CIIP

def test_live_ciip_equals_the_reference(ref, orc):
    _need(ref)
    cp, _ = xc.ciip_picture()
    lines = ic.ciip_differences(cp, ic.run_ciip(ref, "ref", cp), ic.run_ciip(orc, "orc", cp))
    assert not lines, "\n".join(lines)


def test_ciip_premises(orc):
    """XI0: the intra weights 1, 2 and 3 all occur, every unit's marked samples sit on the analytic bounds, and the inter half the oracle
    leaves in the scratch holds both ends of the sample range."""
    cp, units = xc.ciip_picture()
    p = cp.p
    assert set(cc.unit_weights(p).tolist()) == {1, 2, 3}
    n = 0
    for u in units.read:
        for (l, c, inv, b, first, val) in _marked_intermediates(SimpleNamespace(refs=cp.refs, chroma=True, hs=p.hs, vs=p.vs, bd=cp.bd), units, u):
            assert val == b["second"][0 if inv else 1], (u["x"], u["y"], l, c, val, b["second"])
            n += 1
    assert n >= 3 * len(units.read)
    out = ic.run_ciip(orc, "orc", cp)
    inside = out.scratch[cc.region_mask(p)]
    assert np.any(inside == 0) and np.any(inside == (1 << cp.bd) - 1)


# ---------------------------------------------------------------------------------------------------------------- GPM, affine, weights

def test_gpm_premises():
    """XG*: the three mirror types, blend weights 0 .. 8 inside the units (the whole ramp between the tile and its inverse), and every unit
    with the tile in one part and the inverse in the other."""
    mirrors, weights = set(), set()
    for name in xc.GPM:
        pic, units = xc.inter_picture(name)
        for cu, u in zip(pic.gpm, units.read):
            part = int(cu["partition_idx"])
            angle = int(ic.GPM_TABLES["ff_vvc_gpm_angle_idx"][part])
            mirror = int(ic.GPM_TABLES["ff_vvc_gpm_angle_to_mirror"][angle])
            mirrors.add(mirror)
            off_x, off_y = (int(ic.GPM_TABLES[f"ff_vvc_gpm_weights_offset_{k}"][part, 1, 1]) for k in "xy")          # 16x16
            mask = ic.GPM_MASKS[int(ic.GPM_TABLES["ff_vvc_gpm_angle_to_weights_idx"][angle])].reshape(112, 112)
            ys, xs = np.arange(16)[:, None], np.arange(16)[None, :]
            w = mask[off_y + ys, 111 - off_x - xs] if mirror == 1 else mask[111 - off_y - ys, off_x + xs] if mirror == 2 else mask[off_y + ys, off_x + xs]
            weights |= set(np.unique(w).tolist())
            assert u["lists"][0][:2] == u["lists"][1][:2] and u["lists"][0][2] != u["lists"][1][2]
    assert mirrors == {0, 1, 2}, mirrors
    assert weights == set(range(9)), sorted(weights)


def test_affine_premises():
    """XA*: PROF off, on one list and on both; the motion differences sit on both clip bounds in every unit; uni- and bi-predicted units in
    the default, the B-typed and the P-typed weighted slices.  (Whether a unit's model has four or six parameters is decided before this
    stage: the driver reads the sub-blocks' motion from the MvField table, which these pictures fill with one motion per unit so that the
    phase pair is known.)"""
    seen = set()
    for name in xc.AFFINE:
        pic, units = xc.inter_picture(name)
        for cu, u in zip(pic.aff, units.read):
            assert set(np.unique(cu["diff_mv"]).tolist()) == {-xc.DMV_BOUND, xc.DMV_BOUND}
            sl = pic.slices[u["slice"]]
            seen.add((int(cu["prof_flags"]), len(u["lists"]), bool(sl.weighted_bipred), bool(sl.weighted_pred)))
    assert {k[0] for k in seen} == {0, 1, 3}
    assert {k[1:] for k in seen} >= {(1, False, False), (2, False, False), (1, True, False), (2, True, False), (1, False, True)}, sorted(seen)


def test_explicit_weights_sit_on_the_range_ends():
    for flip in (0, 1):
        s = xc.extreme_slices(flip)
        for sl in (s[1], s[2]):
            for c in range(3):
                one = 1 << sl.log2_denom[c > 0]
                pairs = {(sl.weight[l][c][r], sl.offset[l][c][r]) for l in range(2) for r in range(2)}
                assert pairs == {(one + 127, 127), (one - 128, -128), (one - 128, 127), (one + 127, -128)}


def test_every_filter_row_has_its_tile():
    """All rows the inter drivers use — the 15 fractional luma phases of the regular set, the half-sample alternative, the affine 6-tap rows
    and the 31 fractional chroma phases — each against a partner row: on the tile the sample on the period's grid takes the largest
    intermediate `pass_bounds` allows, on the inverse the smallest, and the horizontal-only and vertical-only forms give the one-pass bounds."""
    luma, chroma = xc.filter_rows()
    rows = [(luma[t][f], luma[t][(f * 7) % 15 + 1]) for t in (0, 2) for f in range(1, 16)] + [(luma[1][8], luma[1][8])]
    rows += [(chroma[0][f], chroma[0][(f * 11) % 31 + 1]) for f in range(1, 32)]
    assert len(rows) == 15 + 15 + 1 + 31
    for bd in (8, 10, 12):
        top = (1 << bd) - 1
        for hrow, vrow in rows:
            n = len(hrow)
            ys, xs = np.arange(4 * n)[:, None] % n, np.arange(4 * n)[None, :] % n
            b = xc.pass_bounds(hrow, vrow, 1, 1, bd)
            for inv in (False, True):
                plane = xc.tile_mask(hrow, vrow, "hv", inv)[ys, xs] * top
                assert xc.intermediate(plane, 2 * n, 2 * n, hrow, vrow, 1, 1, bd)[1] == b["second"][0 if inv else 1]
                ph = xc.tile_mask(hrow, vrow, "h", inv)[ys, xs] * top
                assert xc.intermediate(ph, 2 * n, 2 * n, hrow, vrow, 1, 0, bd)[1] == xc.pass_bounds(hrow, vrow, 1, 0, bd)["first"][0 if inv else 1]
                pv = xc.tile_mask(hrow, vrow, "v", inv)[ys, xs] * top
                assert xc.intermediate(pv, 2 * n, 2 * n, hrow, vrow, 0, 1, bd)[1] == xc.pass_bounds(hrow, vrow, 0, 1, bd)["first"][0 if inv else 1]
            assert -(1 << 31) < int(b["second"][0]) * 255 and int(b["second"][1]) * 255 < (1 << 31)          # times the largest weight: inside int


# ---------------------------------------------------------------------------------------------------------------- CC-ALF on matched luma

def test_cc_alf_sums_reach_their_bounds(orc):
    """XF11-XF14: at the chroma samples whose co-located luma sample sits on the 4-grid inside a matched region (away from the picture's
    border and from the luma rows vb - 2 .. vb + 1, where alf_filter_cc folds its rows), the int64 sum of g[k] * (l_k - c) is
    +top * max(P, N) on the tile or its inverse and -top * max(P, N) on the other, for every row a picture uses, and every row of both components is used; per picture some
    corrections saturate at -2^(bd-1) and at 2^(bd-1) - 1 and some stay inside (rows 2 of Cb, 2 and 3 of Cr); where the CTB's chroma ALF is
    off the oracle's sample is clip(chroma + correction)."""
    rows_seen = set()
    for name in xc.ALF_CC:
        fp = xc.filter_picture(name)
        t, bd = fp.t, fp.bd
        top, half = (1 << bd) - 1, 1 << (bd - 1)
        luma = fp.planes[0].astype(np.int64)
        alf = fp.alf.reshape(-1, 8)
        out = pc.run_filter(orc, "orc", fp, "alf")
        ctb, vb = 1 << t.ctb_log2, (1 << t.ctb_log2) - 4
        sums, n = {}, Counter()
        for ry in range(t.height // 16):
            for rx in range(t.width // 16):
                comp, g, inv = xc.cc_region(t, fp.alf, rx, ry)
                if g is None:
                    continue
                rs = ((16 * ry) >> t.ctb_log2) * t.cw + ((16 * rx) >> t.ctb_log2)
                row = int(alf[rs, 5 + comp]) - 1
                g = g.astype(np.int64)
                for Y in range(16 * ry + 4, 16 * ry + 16, 4):
                    if vb - 2 <= Y % ctb <= vb + 1 or Y + 2 >= t.height:
                        continue
                    for X in range(16 * rx + 4, 16 * rx + 16, 4):
                        s = sum(int(g[k]) * int(luma[Y + dy, X + dx] - luma[Y, X]) for k, (dx, dy) in enumerate(xc.CC_TAPS))
                        assert abs(s) == top * xc.cc_bound(g), (name, comp, row, X, Y, s)
                        sums.setdefault((comp, row, inv), set()).add(s)
                        raw = (s + 64) >> 7
                        corr = min(half - 1, max(-half, raw))
                        n["saturated below" if raw < -half else "saturated above" if raw > half - 1 else "inside"] += 1
                        if not alf[rs, comp]:
                            x, y = X >> t.hs, Y >> t.vs
                            want = min(top, max(0, int(fp.planes[comp][y, x]) + corr))
                            assert int(out[comp][y, x]) == want, (name, comp, row, x, y, int(out[comp][y, x]), want)
                            n["outputs checked"] += 1
                            n["sample clip"] += int(not 0 <= int(fp.planes[comp][y, x]) + corr <= top)
        for (comp, row, inv), got in sums.items():
            bound = top * xc.cc_bound(xc.CC_ROWS[comp - 1][row])
            other = sums.get((comp, row, not inv))
            assert len(got) == 1 and other and got | other == {bound, -bound}, (name, comp, row, got, other)
            rows_seen.add((comp, row))
        for key in ("saturated below", "saturated above", "inside", "outputs checked", "sample clip"):
            assert n[key] > 0, (name, key, dict(n))
        print(name, dict(n))
    assert rows_seen == {(comp, row) for comp in (1, 2) for row in range(4)}, sorted(rows_seen)


def test_varying_affine_motion():
    """XA4: inside every unit the sub-blocks' motion differs, in both components, and every luma phase 0 .. 15 occurs in either direction;
    even units carry a four-parameter field (d mvx / dx == d mvy / dy, d mvx / dy == -d mvy / dx), odd units do not."""
    pic, units = xc.inter_picture("XA4")
    phases = [set(), set()]
    for k, u in enumerate(units.read):
        blk = pic.mvf[u["y"] // 4:(u["y"] + 16) // 4, u["x"] // 4:(u["x"] + 16) // 4]
        for l in u["lists"]:
            mv = blk["mv"][:, :, l].astype(np.int64)
            assert len(np.unique(mv[..., 0])) >= 4 and len(np.unique(mv[..., 1])) >= 4
            dx, dy = mv[0, 1] - mv[0, 0], mv[1, 0] - mv[0, 0]
            assert (dx[0] == dy[1] and dy[0] == -dx[1]) == (k % 2 == 0), (k, l, dx, dy)
            for d in range(2):
                phases[d] |= set((mv[..., d] & 15).ravel().tolist())
    assert phases[0] == phases[1] == set(range(16))

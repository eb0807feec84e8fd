"""GPU parity of the chroma bi-prediction launch (vvc355_bipred_chroma_batch) vs orc_bipred_block, every sample of both planes.

The launch gives a wave eight consecutive jobs.  Four Cb/Cr pairs of 4:2:0 8x8 blocks whose 12 x 11 fetch windows lie inside the
planes take the four-pairs-per-wave path (mc_chroma_quad.hpp); every other wave, the tail of the launch included, takes the
one-pair path.  The cases below put both paths, the choice between them and the replicated window edges of the DMVR case
under the oracle: a 64x48 luma picture (chroma 32x24 in 4:2:0) with 16x16 luma blocks on the grid, records filled by hand so
that no luma launch is needed.  In 4:2:0 a block's window is inside the plane for integer positions 1..21 (x) and 1..14 (y).
"""
import ctypes
import functools

import numpy as np
import pytest

import bipred_cases as bc
from conftest import P
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

PW, PH = 64, 48
GRID = [(x, y) for y in range(0, PH, 16) for x in range(0, PW, 16)]          # 12 luma blocks
IN_X, IN_Y = [1, 21, 7, 14, 20, 2, 11, 17], [1, 14, 5, 9, 13, 2]            # integer positions with the window inside, both limits


@functools.lru_cache(maxsize=None)
def planes(bd, fmt):
    """Two reference pictures' chroma planes, shared by every case of one bit depth and format (read only)."""
    hs, vs = fmt
    rng = np.random.default_rng(0xC40A + bd + 64 * hs + 128 * vs)
    refs = [[bc.smooth_picture(rng, PH >> vs, PW >> hs, bd, scale=4) for _ in range(2)] for _ in range(2)]
    for r in refs:
        for p in r:
            p.setflags(write=False)
    return refs


def pair(i, tx=(7, 14), ty=(5, 9), frac=(5, 11, 30, 17), off=None, rfrac=None, dmvr=0, rec=True, wf=None, size=None, pred_flag=(3, 3), hpel=0):
    """One Cb/Cr pair at luma block GRID[i]: reference k is read at integer chroma position (tx[k], ty[k]) plus frac (x0, y0, x1, y1) in
    units of the chroma motion; with off = ((dx0, dy0), (dx1, dy1)) the record's motion is that many whole chroma samples away (and
    has fractions rfrac).  wf = per plane (denom, w0, w1, o0, o1) or None."""
    return dict(i=i % len(GRID), tx=tx, ty=ty, frac=frac, off=off, rfrac=rfrac, dmvr=dmvr, rec=rec, wf=wf, size=size, pred_flag=pred_flag, hpel=hpel)


def run(dev, orc, bd, fmt, pairs, order=None):
    bc.bind_oracle(orc)
    hs, vs = fmt
    isz = 1 if bd == 8 else 2
    cw, ch = PW >> hs, PH >> vs
    refs = planes(bd, fmt)
    want = [np.full((ch, cw), 0x21, refs[0][0].dtype) for _ in range(2)]
    n = len(pairs)
    recs = (abi.BipredResult * max(n, 1))()
    d_out = [batch.DeviceBuffer.from_host(w_) for w_ in want]
    d_refs = [[batch.DeviceBuffer.from_host(np.ascontiguousarray(p)) for p in r] for r in refs]
    jobs = []
    for k, s in enumerate(pairs):
        lx, ly = GRID[s["i"]]
        x, y = lx >> hs, ly >> vs
        w, h = s["size"] or (16 >> hs, 16 >> vs)
        ux, uy = 1 << (4 + hs), 1 << (4 + vs)            # one chroma sample in motion units
        mv, rmv = [], []
        for r in range(2):
            mx, my = (s["tx"][r] - x) * ux + s["frac"][2 * r] % ux, (s["ty"][r] - y) * uy + s["frac"][2 * r + 1] % uy
            mv += [mx, my]
            if s["off"] is None:
                rmv += [mx, my]
            else:
                rf = s["rfrac"] or (0, 0, 0, 0)
                rmv += [(s["tx"][r] + s["off"][r][0] - x) * ux + rf[2 * r] % ux, (s["ty"][r] + s["off"][r][1] - y) * uy + rf[2 * r + 1] % uy]
        for m in range(4):
            recs[k].mv[m] = rmv[m]
        for c in range(2):
            j = abi.BipredJob()
            j.x, j.y, j.w, j.h, j.pic_w, j.pic_h = x, y, w, h, cw, ch
            for m in range(4):
                j.mv[m] = mv[m] if s["rec"] else rmv[m]
            j.chroma, j.hs, j.vs, j.dmvr, j.pred_flag = 1, hs, vs, s["dmvr"], s["pred_flag"][c]
            j.hf_idx = j.vf_idx = s["hpel"]              # 1: the half-sample alternative filter set
            if s["wf"] is not None:
                j.weight_flag = 1
                j.denom, j.w0, j.w1, j.o0, j.o1 = s["wf"][c]
            j.dst_stride = j.ref0_stride = j.ref1_stride = cw * isz
            jobs.append((j, c, k, s["rec"]))
    if order is not None:
        jobs = [jobs[o] for o in order]
    dj = (abi.BipredJob * len(jobs))()
    d_rec = batch.DeviceBuffer.from_host(np.frombuffer(bytes(recs), np.uint8).copy())
    for m, (j, c, k, use_rec) in enumerate(jobs):
        hj = abi.BipredJob.from_buffer_copy(j)
        hj.dst = P(want[c], hj.y * cw + hj.x)
        hj.ref0, hj.ref1 = P(refs[0][c]), P(refs[1][c])
        hj.rec = ctypes.addressof(recs[k]) if use_rec else 0
        orc.orc_bipred_block(bd, ctypes.byref(hj))
        d = abi.BipredJob.from_buffer_copy(j)
        d.dst = d_out[c].ptr + (d.y * cw + d.x) * isz
        d.ref0, d.ref1 = d_refs[0][c].ptr, d_refs[1][c].ptr
        d.rec = d_rec.ptr + 32 * k if use_rec else 0
        dj[m] = d
    d_jobs = batch.jobs_to_device(dj)
    dev.vvc355_bipred_chroma_batch(None, bd, d_jobs.ptr, len(jobs))
    dev.vvc355_stream_sync(None)
    for c in range(2):
        got = d_out[c].to_host(want[c].dtype, want[c].shape)
        bad = np.argwhere(got != want[c])
        assert len(bad) == 0, (f"plane {c + 1}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}: got {got[tuple(bad[0])]} "
                               f"want {want[c][tuple(bad[0])]}; blocks {sorted({(int(b[1]) // 8, int(b[0]) // 8) for b in bad})}")


def inside(i, **kw):
    """A pair whose windows lie inside the planes (4:2:0), positions and fractions varying with i."""
    tx = (IN_X[i % 8], IN_X[(3 * i + 1) % 8])
    ty = (IN_Y[i % 6], IN_Y[(5 * i + 2) % 6])
    frac = (1 + 7 * i, 3 + 5 * i, 31 - 3 * i, 9 + 11 * i)
    return pair(i, tx, ty, frac, hpel=(i >> 1) % 2, **kw)


def weights(rng):
    return tuple((int(rng.integers(0, 8)), *(int(v) for v in rng.integers(-128, 128, size=4))) for _ in range(2))


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("n_pairs", [1, 3, 4, 5, 12])
def test_pair_counts(dev, orc, bd, n_pairs):
    """Tail waves and full waves: 1 and 3 pairs are one short wave, 4 one full wave, 5 a full wave and a tail, 12 three full waves."""
    rng = np.random.default_rng(100 * bd + n_pairs)
    ps = []
    for i in range(n_pairs):
        off = tuple((int(rng.integers(-1, 2)), int(rng.integers(-1, 2))) for _ in range(2))
        ps.append(inside(i, dmvr=1, off=off, rfrac=tuple(int(v) for v in rng.integers(0, 32, size=4)), wf=weights(rng) if i % 3 == 1 else None))
    run(dev, orc, bd, (1, 1), ps)


EDGE = {                    # integer positions (x per reference, y per reference) by pair index
    "interior": lambda i: ((IN_X[i % 8], IN_X[(i + 3) % 8]), (IN_Y[i % 6], IN_Y[(i + 2) % 6])),
    "left": lambda i: ((-i % 7 - 6, 0), (IN_Y[i % 6], 5)),
    "right": lambda i: ((22 + i % 9, 22), (5, IN_Y[i % 6])),
    "top": lambda i: ((IN_X[i % 8], 7), (-(i % 7), 0)),
    "bottom": lambda i: ((7, IN_X[i % 8]), (15 + i % 8, 15)),
    "top_left": lambda i: ((-(i % 5), 0), (0, -(i % 4))),
    "top_right": lambda i: ((22, 23 + i % 8), (-(i % 5), 0)),
    "bottom_left": lambda i: ((0, -(i % 6)), (15 + i % 7, 16)),
    "bottom_right": lambda i: ((22 + i % 8, 29), (15, 16 + i % 7)),
    "far": lambda i: (((-125, 125)[i % 2], (125, -125)[(i >> 1) % 2]), ((93, -93)[(i >> 1) % 2], (-93, 93)[i % 2])),
}


@pytest.mark.parametrize("dmvr", [0, 1])
@pytest.mark.parametrize("where", list(EDGE))
def test_motion(dev, orc, where, dmvr):
    """Windows inside the planes, across each edge and corner, and far outside (+-4000 in motion units): dmvr = 0 reads around the motion
    itself (every other pair without a record), dmvr = 1 around the unrefined block with the record one sample away."""
    ps = []
    for i in range(12):
        tx, ty = EDGE[where](i)
        frac = (1 + 7 * i, 3 + 5 * i, 31 - 3 * i, 9 + 11 * i)
        if dmvr:
            ps.append(pair(i, tx, ty, frac, dmvr=1, off=((1 - i % 3, i % 3 - 1), ((i >> 1) % 3 - 1, 1 - (i >> 2) % 3)), rfrac=frac[::-1]))
        else:
            ps.append(pair(i, tx, ty, frac, rec=bool(i % 2)))
    run(dev, orc, 10, (1, 1), ps)


@pytest.mark.parametrize("dmvr", [0, 1])
@pytest.mark.parametrize("zero", ["x", "y", "xy"])
def test_zero_fractions(dev, orc, zero, dmvr):
    """Whole-sample motion in x only, in y only and in both: copy / h / v / hv, per reference in every combination."""
    ps = []
    for i in range(12):
        f = [1 + 7 * i % 31, 2 + 5 * i % 30, 31 - i, 3 + 2 * i]
        both = i % 3            # 0: both references, 1: reference 0 only, 2: reference 1 only
        for r in range(2):
            if both == 0 or both == r + 1:
                if "x" in zero: f[2 * r] = 0
                if "y" in zero: f[2 * r + 1] = 0
        kw = dict(dmvr=1, off=((i % 3 - 1, 0), (0, 1 - i % 3)), rfrac=tuple(f)) if dmvr else {}
        ps.append(inside(i, **kw))
        ps[-1]["frac"] = tuple(f)
    run(dev, orc, 10, (1, 1), ps)


OFFS9 = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("frac", [0, 1])
@pytest.mark.parametrize("variant", ["unit", "two", "three"])
def test_dmvr_offsets(dev, orc, variant, frac, bd):
    """dmvr = 1 with the record's motion every whole chroma offset of {-1, 0, 1}^2 away from the job's, with and without a fraction: the
    reads one sample outside the window are replicated edge samples.  "two" adds offsets of two samples (still the quad path), "three"
    one of three samples, which sends its wave down the one-pair path."""
    extra = {"unit": [(1, -1), (-1, 1), (0, 0)], "two": [(2, -2), (-2, 2), (-2, -2)], "three": [(3, 0), (0, -3), (2, 1)]}[variant]
    offs = OFFS9 + extra
    ps = []
    for i in range(12):
        o0, o1 = offs[i], offs[(i * 5 + 3) % 12] if variant != "three" else offs[(i + 4) % 12]
        rf = (3 + i, 29 - 2 * i, 16, 1 + 2 * i) if frac else (0, 0, 0, 0)
        ps.append(inside(i, dmvr=1, off=(o0, o1), rfrac=rf))
    run(dev, orc, bd, (1, 1), ps)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_weights_differ_per_plane(dev, orc, bd):
    rng = np.random.default_rng(0xBEEF + bd)
    ps = [inside(i, dmvr=i % 2, off=((0, 1), (-1, 0)) if i % 2 else None, rfrac=(9, 0, 0, 21), wf=weights(rng)) for i in range(12)]
    ps[5]["wf"] = ((7, 127, -128, 127, 127), (0, -128, 127, -128, -128))          # the extremes
    run(dev, orc, bd, (1, 1), ps)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("odd", ["uni", "small", "order", "edge"])
def test_mixed_waves(dev, orc, odd, bd):
    """One pair of the first wave is not a quad candidate, the other three are: the whole wave takes the one-pair path.  The second wave
    is four candidates."""
    ps = [inside(i, dmvr=1, off=((1, 0), (0, -1)), rfrac=(4, 8, 15, 16)) for i in range(8)]
    order = None
    if odd == "uni":
        ps[2] = inside(2, pred_flag=(1, 2))                             # uni-predicted jobs: no dmvr
    elif odd == "small":
        ps[1] = inside(1, size=(4, 4))
    elif odd == "order":
        order = [0, 1, 2, 4, 3, 5, 6, 7] + list(range(8, 16))           # Cb, Cb, Cr, Cr
    else:
        ps[3] = pair(3, (0, 14), (5, 9), dmvr=1, off=((1, 0), (0, -1)), rfrac=(4, 8, 15, 16))      # window column -1
    run(dev, orc, bd, (1, 1), ps, order)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("fmt", [(1, 0), (0, 0)])
def test_other_formats(dev, orc, fmt, bd):
    """4:2:2 (8x16 blocks) and 4:4:4 (16x16): always the one-pair path."""
    ps = []
    for i in range(12):
        x, y = GRID[i][0] >> fmt[0], GRID[i][1] >> fmt[1]
        ps.append(pair(i, (x + i % 5 - 2, x - i % 3), (y - i % 4, y + i % 6 - 2), (1 + 7 * i, 3 + 5 * i, 61 - 3 * i, 9 + 11 * i),
                       dmvr=i % 2, off=((1, -1), (0, 1)) if i % 2 else None, rfrac=(5, 0, 0, 13)))
    run(dev, orc, bd, fmt, ps)

"""vvc355_affine_batch against the oracle's orc_affine_block on a 48x40 picture, case by case for what the kernel's mapping can get wrong:
the vector window fetch against the clamped one (windows inside, over each border and corner, and on both sides of the fetch's own
limits), the one-formula filter (zero and non-zero fractions, fractions >= 8 for the PROF ring's offset), slots against lists
(pred_flag 1, 2, 3; PROF on neither, one or both lists), the output formulas (weighted or not, with and without the forward map), groups
missing from a wave, and neighbours in the job array that have nothing to do with each other.  Every launch compares the whole plane."""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import P, rand_pixels
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

PW, PH = 48, 40
NBLK = (PW // 4) * (PH // 4)
# integer window origins (block position + whole-sample motion): far outside, one short of the vector fetch's limit, on it, well inside
OXS = [-9, 2, 3, 20, PW - 9, PW - 8, PW + 2]          # the fetch reads columns ox - 3 .. ox + 8
OYS = [-9, 2, 3, 16, PH - 8, PH - 7, PH + 5]          # and rows oy - 3 .. oy + 7
FRACS = [(0, 0), (9, 0), (0, 12), (3, 5), (8, 15), (15, 8)]


class Picture:
    def __init__(self, orc, bd, seed):
        orc.orc_affine_block.argtypes = [ctypes.c_int, ctypes.POINTER(abi.AffineJob)]
        orc.orc_affine_block.restype = None
        self.orc, self.bd, self.isz = orc, bd, 1 if bd == 8 else 2
        self.rng = np.random.default_rng(seed)
        self.refs = [rand_pixels(self.rng, (PH, PW), bd) for _ in range(2)]
        self.lut = np.sort(self.rng.integers(0, 1 << bd, size=1 << bd)).astype(self.refs[0].dtype)
        self.d_refs = [batch.DeviceBuffer.from_host(r) for r in self.refs]
        self.d_lut = batch.DeviceBuffer.from_host(self.lut)

    def launch(self, dev, specs, n=None):
        """specs: (pred_flag, prof0, prof1, weighted, lut, (ox0, oy0, fx0, fy0), (ox1, oy1, fx1, fy1)), at most one per 4x4 block of the
        picture; destinations are dealt at random.  Only the first n are launched and expected; the array holds them all."""
        assert len(specs) <= NBLK
        n = len(specs) if n is None else n
        rng, bd, isz = self.rng, self.bd, self.isz
        want = np.full((PH, PW), 0x17, self.refs[0].dtype)
        d_out = batch.DeviceBuffer.from_host(want)
        dmv = rng.integers(-32, 33, size=(len(specs), 2, 2, 16)).astype(np.int16)
        d_dmv = batch.DeviceBuffer.from_host(dmv)
        arr = (abi.AffineJob * len(specs))()
        for i, (blk, (pf, p0, p1, wf, lut, m0, m1)) in enumerate(zip(rng.permutation(NBLK), specs)):
            x, y = int(blk % (PW // 4)) * 4, int(blk // (PW // 4)) * 4
            j = abi.AffineJob()
            j.x, j.y, j.pic_w, j.pic_h = x, y, PW, PH
            j.pred_flag, j.prof0, j.prof1, j.weight_flag = pf, p0, p1, wf
            for k, (ox, oy, fx, fy) in enumerate((m0, m1)):
                j.mv[2 * k], j.mv[2 * k + 1] = (ox - x) * 16 + fx, (oy - y) * 16 + fy
            j.denom = int(rng.integers(0, 8))
            j.w0, j.w1, j.o0, j.o1 = (int(v) for v in rng.integers(-128, 128, size=4))
            j.dst_stride = j.ref0_stride = j.ref1_stride = PW * isz
            if i < n:
                hj = abi.AffineJob.from_buffer_copy(j)
                hj.dst, hj.ref0, hj.ref1 = P(want, y * PW + x), P(self.refs[0]), P(self.refs[1])
                hj.diff_mv, hj.lmcs_lut = P(dmv, i * 64), P(self.lut) if lut else 0
                self.orc.orc_affine_block(bd, ctypes.byref(hj))
            j.dst, j.ref0, j.ref1 = d_out.ptr + (y * PW + x) * isz, self.d_refs[0].ptr, self.d_refs[1].ptr
            j.diff_mv, j.lmcs_lut = d_dmv.ptr + i * 128, self.d_lut.ptr if lut else 0
            arr[i] = j
        d_jobs = batch.jobs_to_device(arr)
        dev.vvc355_affine_batch(None, bd, d_jobs.ptr, n)
        dev.vvc355_stream_sync(None)
        got = d_out.to_host(want.dtype, want.shape)
        bad = np.argwhere(got != want)
        if len(bad):
            by, bx = bad[0].tolist()
            hit = [(s, list(a.mv)) for s, a in zip(specs, arr) if a.x <= bx < a.x + 4 and a.y <= by < a.y + 4]
            raise AssertionError(f"{len(bad)} samples differ, first at (y, x) = ({by}, {bx}): job {hit}")
        assert n == 0 or np.any(want != 0x17)

    def launch_all(self, dev, specs):
        for k in range(0, len(specs), NBLK - 3):            # a last wave with a group missing in every launch
            self.launch(dev, specs[k:k + NBLK - 3])


MODES = list(itertools.product((1, 2, 3), (0, 1), (0, 1), (0, 1), (0, 1)))       # pred_flag, prof0, prof1, weighted, lut


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_windows_inside_over_borders_and_corners(dev, orc, bd):
    """Every pair of the window origins above (inside, beyond each border, beyond each corner, and the four positions next to the vector
    fetch's limits) with every kind of fraction; the second list's window is another one of the set."""
    pic = Picture(orc, bd, 0xAFF0 + bd)
    pos = list(itertools.product(OXS, OYS))
    specs = []
    for k, ((ox, oy), (fx, fy)) in enumerate(itertools.product(pos, FRACS[:4])):
        ox1, oy1 = pos[(7 * k + 3) % len(pos)]
        fx1, fy1 = FRACS[(k + 2) % len(FRACS)]
        specs.append(MODES[k % len(MODES)] + ((ox, oy, fx, fy), (ox1, oy1, fx1, fy1)))
    pic.launch_all(dev, specs)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_lists_prof_weights_map_and_fractions(dev, orc, bd):
    """pred_flag 1 / 2 / 3 x PROF on neither, one or both lists x weighted or not x forward map or not, each with zero and non-zero
    fractions in all four combinations and fractions >= 8; windows at random, about a third of them over a border."""
    pic = Picture(orc, bd, 0xAFF8 + bd)
    specs = []
    for mode, (fx, fy) in itertools.product(MODES, FRACS):
        m = [(int(pic.rng.integers(-2, PW - 4)), int(pic.rng.integers(-2, PH - 3))) for _ in range(2)]
        specs.append(mode + ((m[0][0], m[0][1], fx, fy), (m[1][0], m[1][1], fy, fx)))
    order = pic.rng.permutation(len(specs))
    pic.launch_all(dev, [specs[int(i)] for i in order])


@pytest.mark.parametrize("n", [1, 3, 5, 17])
@pytest.mark.parametrize("bd", [8, 10])
def test_waves_with_absent_groups(dev, orc, bd, n):
    """n_jobs that leave groups of the last wave without a job; the array goes on beyond n_jobs with jobs that must not run."""
    pic = Picture(orc, bd, 0xAFFC + bd + n)
    specs = []
    for k in range(n + 9):
        m = [(int(pic.rng.integers(-6, PW + 2)), int(pic.rng.integers(-6, PH + 2)), int(pic.rng.integers(0, 16)), int(pic.rng.integers(0, 16))) for _ in range(2)]
        specs.append(MODES[int(pic.rng.integers(0, len(MODES)))] + (m[0], m[1]))
    pic.launch(dev, specs, n)

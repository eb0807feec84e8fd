"""vvc355_lmcs_chroma_resid_batch's mapping against the oracle's orc_lmcs_chroma_resid_block: sixty-four slots per workgroup of eight
waves, the slots' four-sample units dealt over all lanes (256 units per wave and step), one aligned vector read-modify-write per unit.
What the mapping can get wrong is which unit belongs to which slot (empty slots between full ones, whole workgroups of empty slots,
blocks of very different sizes side by side, the end of the array inside a workgroup) and where a unit lies in its block (every shape,
blocks that end at the plane's right and bottom edge, planes whose rows are not aligned to a unit).  Every case compares both chroma
planes whole."""
import ctypes

import numpy as np
import pytest

import recon_cases
from conftest import P, rand_pixels
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

PW, PH = 192, 128                  # luma; 4:2:0 chroma planes of 96 x 64
CW, CH = PW // 2, PH // 2
JOINTS = [0, 1, 1 | 2, 1 | 4, 1 | 2 | 4, 8, 8 | 1, 8 | 1 | 2, 8 | 1 | 4, 8 | 1 | 2 | 4, 8 | 16, 8 | 16 | 1, 8 | 16 | 1 | 2, 8 | 16 | 1 | 4, 8 | 16 | 1 | 2 | 4]


def layout():
    """Disjoint (x, y, w, h) chroma blocks covering the 96 x 64 plane: 2x8, 4x4, 4x16, 8x8, 16x4 and 32x32, among them blocks that end at
    the right edge, at the bottom edge and in the bottom right corner."""
    b = [(0, 0, 32, 32), (32, 32, 32, 32), (64, 32, 32, 32)]
    b += [(32 + 8 * i, 0, 8, 8) for i in range(4)] + [(32 + 4 * i, 8, 4, 16) for i in range(8)]
    b += [(32 + 16 * i, 24, 16, 4) for i in range(2)] + [(32 + 4 * i, 28, 4, 4) for i in range(8)]
    b += [(64 + 2 * i, 0, 2, 8) for i in range(16)] + [(64 + 8 * i, 8, 8, 8) for i in range(4)] + [(64 + 16 * i, 16, 16, 4) for i in range(2)]
    b += [(64 + 8 * i, 20, 8, 8) for i in range(4)] + [(64 + 4 * i, 28, 4, 4) for i in range(8)]
    b += [(4 * i, 32, 4, 16) for i in range(8)] + [(16 * i, 48, 16, 4) for i in range(2)] + [(2 * i, 52, 2, 8) for i in range(16)]
    b += [(4 * i, 60, 4, 4) for i in range(8)]
    cover = np.zeros((CH, CW), np.int32)
    for (x, y, w, h) in b:
        cover[y:y + h, x:x + w] += 1
    assert np.all(cover == 1)
    return b


class Picture:
    """Luma, two chroma planes (rows of CW + pad samples), a scale table, the model, and the device copies."""

    def __init__(self, orc, bd, seed, pad=0):
        orc.orc_lmcs_chroma_resid_block.argtypes = [ctypes.c_int, ctypes.POINTER(abi.LmcsResidJob), ctypes.POINTER(abi.LmcsModel)]
        orc.orc_lmcs_chroma_resid_block.restype = None
        self.orc, self.bd, self.isz = orc, bd, 1 if bd == 8 else 2
        self.rng = np.random.default_rng(seed)
        self.luma = rand_pixels(self.rng, (PH, PW), bd)
        self.cstride = CW + pad
        self.chroma = [rand_pixels(self.rng, (CH, self.cstride), bd) for _ in range(2)]
        self.want = [p.copy() for p in self.chroma]
        self.model = recon_cases.ReconWork.lmcs_model(self.rng, bd)
        self.table = self.rng.integers(1024, 4096, size=6).astype(np.int16)
        self.resid = self.rng.integers(-(1 << (bd + 1)), 1 << (bd + 1), size=CW * CH * 2 + 64).astype(np.int32)      # room for every block of both planes
        self.d_luma = batch.DeviceBuffer.from_host(self.luma)
        self.d_c = [batch.DeviceBuffer.from_host(p) for p in self.chroma]
        self.d_model = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.model), np.uint8))
        self.d_table = batch.DeviceBuffer.from_host(self.table)
        self.d_res = batch.DeviceBuffer.from_host(self.resid)
        self.off = 0

    def job(self, c, x, y, w, h, joint, apply=True):
        """The device job of one block; with apply, the oracle adds it to the expected planes."""
        j = abi.LmcsResidJob()
        j.w, j.h, j.joint = w, h, joint
        cux, cuy = min(2 * x + int(self.rng.integers(0, 2)) * 8, PW - 1), 2 * y
        j.x_vpdu, j.y_vpdu, j.pic_w, j.pic_h, j.size_y = cux & ~63, cuy & ~63, PW, PH, 64
        j.avail_l, j.avail_t = int(j.x_vpdu > 0 and self.rng.random() < 0.8), int(j.y_vpdu > 0 and self.rng.random() < 0.8)
        unit = (j.y_vpdu // 64) * 3 + j.x_vpdu // 64
        off = self.off
        self.off += (w * h + 3) & ~3
        if apply:
            hj = abi.LmcsResidJob.from_buffer_copy(j)
            hj.dst, hj.dst_stride, hj.resid = P(self.want[c], y * self.cstride + x), self.cstride * self.isz, P(self.resid, off)
            hj.luma, hj.luma_stride = (P(self.table, unit), 0) if joint & 16 else (P(self.luma), PW * self.isz)
            self.orc.orc_lmcs_chroma_resid_block(self.bd, ctypes.byref(hj), ctypes.byref(self.model))
        j.dst, j.dst_stride, j.resid = self.d_c[c].ptr + (y * self.cstride + x) * self.isz, self.cstride * self.isz, self.d_res.ptr + off * 4
        j.luma, j.luma_stride = (self.d_table.ptr + unit * 2, 0) if joint & 16 else (self.d_luma.ptr, PW * self.isz)
        return j

    def run_and_check(self, dev, slots, n=None):
        n = len(slots) if n is None else n
        arr = (abi.LmcsResidJob * max(len(slots), 1))()
        for i, s in enumerate(slots):
            if s is not None:
                arr[i] = s
        d_jobs = batch.jobs_to_device(arr)
        dev.vvc355_lmcs_chroma_resid_batch(None, self.bd, d_jobs.ptr, n, self.d_model.ptr)
        dev.vvc355_stream_sync(None)
        for c in range(2):
            got = self.d_c[c].to_host(self.want[c].dtype, self.want[c].shape)
            bad = np.argwhere(got != self.want[c])
            assert len(bad) == 0, f"component {c + 1}: {len(bad)} samples differ, first at (y, x) = {bad[0].tolist()}"


def mixed_jobs(pic, blocks, upto=None):
    """One job per block in a shuffled order (neighbours in the array are unrelated blocks), planes alternating, joint cycling; the oracle
    applies the first `upto` of them."""
    order = pic.rng.permutation(len(blocks))
    upto = len(blocks) if upto is None else upto
    return [pic.job(k % 2, *blocks[int(i)], JOINTS[k % len(JOINTS)], apply=k < upto) for k, i in enumerate(order)]


@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_every_shape_with_empty_slots_between(dev, orc, bd, pad):
    """Every shape, every joint mode, table and derived scales, blocks at the right and bottom edges; between the full slots runs of 0, 2
    and 7 empty ones.  pad = 2 makes rows of 98 samples: at 8 bit a row is no multiple of 4 bytes, at 10 / 12 bit none of 8, and the blocks
    take their samples one by one."""
    pic = Picture(orc, bd, 0x1E40 + bd + pad, pad)
    jobs = mixed_jobs(pic, layout())
    slots = []
    for k, j in enumerate(jobs):
        slots += [j] + [None] * (0, 2, 7)[k % 3]
    assert len(slots) % 16 != 0 and len(slots) > 256
    assert {(j.w, j.h) for j in jobs} == {(2, 8), (4, 4), (4, 16), (8, 8), (16, 4), (32, 32)}
    pic.run_and_check(dev, slots)
    assert all(np.any(pic.want[c] != pic.chroma[c]) for c in range(2))


@pytest.mark.parametrize("bd", [8, 10])
def test_runs_of_only_empty_slots(dev, orc, bd):
    """Several workgroups' slots empty at the start, two more between full ones, an empty run shorter than a workgroup's, empty slots at the end."""
    pic = Picture(orc, bd, 0x1E50 + bd)
    jobs = mixed_jobs(pic, layout())
    slots = [None] * 300 + jobs[:20] + [None] * 140 + jobs[20:23] + [None] * 61 + jobs[23:] + [None] * 70
    assert len(slots) % 16 != 0
    pic.run_and_check(dev, slots)


@pytest.mark.parametrize("bd", [8, 10])
def test_large_blocks_first_in_both_planes(dev, orc, bd):
    """Every block of the layout in both planes, sorted by size as the transform-block builder leaves them, no empty slots: the first
    workgroup's 64 slots hold the six 32x32 blocks and more than 2048 units, so its waves take a second step."""
    pic = Picture(orc, bd, 0x1E80 + bd)
    blocks = sorted(layout(), key=lambda b: -b[2] * b[3])
    slots = [pic.job(c, *b, JOINTS[(2 * k + c) % len(JOINTS)]) for k, b in enumerate(blocks) for c in range(2)]
    units = [j.w * j.h if j.w < 4 else j.w * j.h // 4 for j in slots[:64]]
    assert sum(units) > 2048 and len(slots) % 16 != 0
    pic.run_and_check(dev, slots)


@pytest.mark.parametrize("n", [0, 37, 256])
def test_nothing_but_empty_slots(dev, orc, n):
    pic = Picture(orc, 10, 0x1E60 + n)
    pic.run_and_check(dev, [None] * n)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("n", [1, 5, 17, 63, 65, 250, 257])
def test_job_count_ends_inside_a_workgroup(dev, orc, bd, n):
    """n_jobs on both sides of a workgroup's 64 slots and of multiples of it; the array goes on with full slots beyond n_jobs that must not be
    touched."""
    pic = Picture(orc, bd, 0x1E70 + bd + n)
    blocks = layout()
    while len(blocks) < 270:                                         # more blocks than n: quarter the ones of 8x8 and more
        x, y, w, h = blocks.pop(next(i for i, b in enumerate(blocks) if b[2] >= 8 and b[3] >= 8))
        blocks += [(x, y, w // 2, h // 2), (x + w // 2, y, w // 2, h // 2), (x, y + h // 2, w // 2, h // 2), (x + w // 2, y + h // 2, w // 2, h // 2)]
    slots = mixed_jobs(pic, blocks, upto=n)
    assert len(slots) > n and n % 16 != 0
    pic.run_and_check(dev, slots, n)

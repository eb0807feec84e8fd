"""CPU: the host packer vvc355_levels_pack (ffvvc_amd/host/levels_pack.c) against the numpy restatement in levels_cases.py."""
import ctypes

import numpy as np
import pytest

import levels_cases as lc
from ffvvc_amd import abi

# every block size a VVC transform block takes, 1x16 / 16x1 ISP parts and 2xN / Nx2 included, plus the other small ones the format admits
SIZES = [(lw, lh) for lw in range(7) for lh in range(7) if (1 << lw) * (1 << lh) >= 4]


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def run_pack(lib, c, first=0):
    h, w = c.shape
    c = np.ascontiguousarray(c, np.int32)
    out = np.full(64 * 16 + 16, 0x5A5A, np.uint16).view(np.int16)
    rec = abi.TbLevels()
    n = lib.vvc355_levels_pack(c.ctypes.data, int(np.log2(w)), int(np.log2(h)), out.ctypes.data, ctypes.byref(rec), first)
    return n, out, rec


def check_against_numpy(lib, c, first):
    h, w = c.shape
    n, out, rec = run_pack(lib, c, first)
    want = lc.pack(c)
    assert want is not None
    mask, groups = want
    assert (n, rec.groups, rec.first, rec.flags) == (len(groups), mask, first, 0), (w, h)
    assert np.array_equal(out[:n * 16].reshape(-1, 16), groups), (w, h)
    assert np.all(out[n * 16:].view(np.uint16) == 0x5A5A)             # nothing written past the block's groups
    assert np.array_equal(lc.unpack(rec.groups, out, 0, w, h), c)      # and the restatement's unpacker inverts it
    return n


def test_tb_levels_layout():
    assert ctypes.sizeof(abi.TbLevels) == 16
    assert abi.TbLevels.first.offset == 8 and abi.TbLevels.flags.offset == 12


def test_pack_windows_every_size(lib):
    rng = np.random.default_rng(0x5EED1E00)
    coded = 0
    for (lw, lh) in SIZES:
        w, h = 1 << lw, 1 << lh
        for rep in range(6):
            nzw, nzh = int(rng.integers(1, min(w, 32) + 1)), int(rng.integers(1, min(h, 32) + 1))
            c = lc.windowed_block(rng, w, h, nzw, nzh)
            if rep == 0 and w <= 32 and h <= 32:
                c = lc.windowed_block(rng, w, h, w, h, bits=15)           # transform-skip-like: the whole block, full int16 range
                c[0, 0] = -32768
            coded += check_against_numpy(lib, c, int(rng.integers(0, 1 << 32)))
    assert coded > 1000


def test_pack_empty_and_full_grid(lib):
    for (w, h) in ((4, 4), (2, 8), (64, 64), (16, 1)):
        n, out, rec = run_pack(lib, np.zeros((h, w), np.int32), 77)
        assert (n, rec.groups, rec.first, rec.flags) == (0, 0, 77, 0)
        assert np.all(out.view(np.uint16) == 0x5A5A)
    rng = np.random.default_rng(0x5EED1E01)
    for (w, h) in ((32, 32), (64, 64), (64, 32)):
        c = np.zeros((h, w), np.int32)
        c[:32, :32] = rng.integers(1, 100, size=(32, 32))
        n, out, rec = run_pack(lib, c, 5)
        assert n == 64 and rec.groups == (1 << 64) - 1                  # the 8 x 8 grid: bit 63 is the tile at (28, 28)
        assert np.array_equal(out[63 * 16:64 * 16].reshape(4, 4), c[28:32, 28:32])
        check_against_numpy(lib, c, 5)


@pytest.mark.parametrize("w,h,y,x,v,err", [
    (16, 16, 3, 5, 32768, abi.LEVELS_E_RANGE), (8, 4, 0, 0, -32769, abi.LEVELS_E_RANGE), (2, 8, 7, 1, 1 << 20, abi.LEVELS_E_RANGE),
    (64, 64, 0, 32, 1, abi.LEVELS_E_ZERO_OUT), (64, 64, 40, 3, -1, abi.LEVELS_E_ZERO_OUT), (64, 16, 15, 63, 9, abi.LEVELS_E_ZERO_OUT),
])
def test_pack_errors(lib, w, h, y, x, v, err):
    c = np.zeros((h, w), np.int32)
    c[0, 0] = 3
    c[y, x] = v
    n, out, rec = run_pack(lib, c, 12)
    assert n == err
    assert (rec.groups, rec.first, rec.flags) == (0, 12, abi.LEVELS_INT32)
    assert np.all(out.view(np.uint16) == 0x5A5A)                         # a block that stays on the int32 path leaves the stream alone
    assert lc.pack(c) is None

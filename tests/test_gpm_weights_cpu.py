"""CPU: the geometric-partition tables and weight masks of the library against the reference's, held as data in
tests/golden/gpm_tables.npz (tools/ref_gpm_tables.py).  The library computes its masks from the standard's closed form; here every
partition, block size and chroma subsampling is checked to get the weights pred_gpm_blk (vvc_inter.c:466-527) addresses in
ff_vvc_gpm_weights: the offset tables, the mirror type and the signed steps."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from ffvvc_amd import abi

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "gpm_tables.npz"))
SIZES = [(w, h) for w in (8, 16, 32, 64) for h in (8, 16, 32, 64) if w < 8 * h and h < 8 * w]


@pytest.fixture(scope="module")
def lib():
    return abi.load()


def reference_weights(part, cb_w, cb_h, hs, vs):
    """pred_gpm_blk's addressing of the fixture's masks (vvc_inter.c:473-497)."""
    angle = int(GOLDEN["ff_vvc_gpm_angle_idx"][part])
    widx = int(GOLDEN["ff_vvc_gpm_angle_to_weights_idx"][angle])
    mirror = int(GOLDEN["ff_vvc_gpm_angle_to_mirror"][angle])
    w, h = cb_w.bit_length() - 4, cb_h.bit_length() - 4                  # av_log2(cb) - 3
    off_x = int(GOLDEN["ff_vvc_gpm_weights_offset_x"][part, h, w])
    off_y = int(GOLDEN["ff_vvc_gpm_weights_offset_y"][part, h, w])
    step_x, step_y = 1 << hs, 112 << vs
    if mirror == 0:
        first = off_y * 112 + off_x
    elif mirror == 1:
        step_x, first = -step_x, off_y * 112 + 111 - off_x
    else:
        step_y, first = -step_y, (111 - off_y) * 112 + off_x
    ys, xs = np.mgrid[0:cb_h >> vs, 0:cb_w >> hs]
    return GOLDEN["ff_vvc_gpm_weights"][widx][first + ys * step_y + xs * step_x]


def test_partition_tables_match_fixture(lib):
    for name, ct, n in (("angle_idx", ctypes.c_uint8, 64), ("distance_idx", ctypes.c_uint8, 64), ("distance_lut", ctypes.c_int8, 32)):
        got = np.array((ct * n).in_dll(lib, "vvc355_tab_gpm_" + name)[:])
        assert np.array_equal(got, GOLDEN["ff_vvc_gpm_" + name].astype(got.dtype)), name


@pytest.mark.parametrize("hs,vs", [(0, 0), (1, 1), (1, 0)])
def test_weights_match_reference_masks(lib, hs, vs):
    mirrors = set()
    for part in range(64):
        mirrors.add(int(GOLDEN["ff_vvc_gpm_angle_to_mirror"][GOLDEN["ff_vvc_gpm_angle_idx"][part]]))
        for cb_w, cb_h in SIZES:
            for sx, sy in ((0, 0), (hs, vs)):                             # luma, then the chroma of this format
                got = np.zeros((cb_h >> sy, cb_w >> sx), np.uint8)
                lib.vvc355_gpm_weights(part, cb_w, cb_h, sx, sy, got.ctypes.data)
                want = reference_weights(part, cb_w, cb_h, sx, sy)
                bad = np.argwhere(got != want)
                assert len(bad) == 0, f"partition {part}, {cb_w}x{cb_h}, (hs, vs) = ({sx}, {sy}): first difference at (y, x) = {bad[0].tolist()}"
    assert mirrors == {0, 1, 2}

"""GPU parity of the RECON pass where its walk reads plans instead of commands (ffvvc_amd/csrc/recon_plan.hpp): the seams between the
windows of 64 commands a plan is made in, the strip path at a CTU's top edge with wide-angle and multi-reference-line blocks, and the
commands in HBM, which the plans must never reach.  Bit-exact against orc_recon_frame_pass, two passes per case (test_recon_gpu.run_case)."""
import numpy as np
import pytest

import recon_cases
from ffvvc_amd import abi, batch
from test_recon_gpu import run_case

pytestmark = pytest.mark.gpu


@pytest.fixture
def uploads(monkeypatch):
    """Every host array run_case uploads, with its device buffer (kept alive until the test ends)."""
    seen = []
    plain = batch.DeviceBuffer.from_host.__func__

    def from_host(cls, arr):
        buf = plain(cls, arr)
        seen.append((np.array(arr, copy=True), buf))
        return buf
    monkeypatch.setattr(batch.DeviceBuffer, "from_host", classmethod(from_host))
    return seen


def check_commands_untouched(uploads, work):
    """(c) After the pass, bytes 0-33 of every command in HBM are what was uploaded: the plan lives in LDS, only the pad bytes are the pass's."""
    mine = [(a, b) for a, b in uploads if a.dtype == np.uint8 and a.nbytes == len(work.cmds) * 40]
    assert len(mine) == 1
    sent, buf = mine[0]
    back = buf.to_host(np.uint8, sent.shape)
    assert np.array_equal(back.reshape(-1, 40)[:, :34], sent.reshape(-1, 40)[:, :34])


def seams(work):
    """Per CTU and wave (luma / chroma commands, MARKs aside): Cb / Cr twins at command indices 63 | 64 (mod 64) of their CTU, PREDs whose
    RESID is the first command of the next window, CCLMs that are the first command of a window."""
    twin = resid = cclm = 0
    for ctu in work.ctus:
        n = int(ctu["n_cmd"])
        c = work.cmds[int(ctu["first_cmd"]):int(ctu["first_cmd"]) + n]
        kind, c_idx = c["kind"], c["c_idx"]
        for wave in (0, 1):
            idx = [i for i in range(n) if kind[i] != abi.RECON_MARK and (c_idx[i] > 0) == (wave == 1)]
            for a, b in zip(idx, idx[1:]):
                twin += int(kind[a] == kind[b] == abi.RECON_PRED and c_idx[a] == 1 and c_idx[b] == 2 and b == a + 1 and a % 64 == 63)
                resid += int(kind[a] == abi.RECON_PRED and kind[b] == abi.RECON_RESID and b % 64 == 0)
            cclm += sum(1 for i in idx if kind[i] == abi.RECON_CCLM and i % 64 == 0 and i > 0)
    return twin, resid, cclm


def test_window_seams(dev, orc, uploads):
    """(a) 3 x 2 CTUs of 128x128 (the last column 8 samples wide, the lower row 8 tall) split down to 4x4: thousands of commands per CTU, and the seed puts a twin pair,
    a PRED | RESID pair and a CCLM across / at window borders — counted on the CPU before the launch."""
    seed, kw = 0x5EED1000, dict(intra_frac=1.0, min_cu=4, split=(0.95, 0.8), coded_p=0.9)
    probe = recon_cases.ReconWork(np.random.default_rng(seed), 264, 136, 7, 1, 1, **kw)
    twin, resid, cclm = seams(probe)
    assert twin > 0 and resid > 0 and cclm > 0 and probe.ctus["n_cmd"].max() > 128
    work, changed = run_case(dev, orc, np.random.default_rng(seed), 10, 264, 136, 7, (1, 1), **kw)
    assert np.array_equal(work.cmds, probe.cmds)
    assert changed > 264 * 136 // 2
    check_commands_untouched(uploads, work)


@pytest.mark.parametrize("bd,ctb_log2,lmcs", [(8, 5, False), (10, 6, True), (12, 7, False)])
def test_strip_wide_angle_and_reference_lines(dev, orc, uploads, bd, ctb_log2, lmcs):
    """(b) The all-intra picture of test_recon_gpu on the LDS-tile walk for every CTU size: blocks on a CTU's top edge read the rows above
    from the strip, wide-angle modes among them; blocks below it pick reference lines 1 and 2."""
    rng = np.random.default_rng(0x5EED1100 + bd + 16 * ctb_log2)
    work, changed = run_case(dev, orc, rng, bd, 456, 264, ctb_log2, (1, 1), intra_frac=1.0, n_slices=3 if ctb_log2 < 7 else 1, tiles=ctb_log2 == 6, lmcs=lmcs)
    c = work.cmds[work.cmds["kind"] == abi.RECON_PRED]
    top = c[(c["y0"] & ((1 << ctb_log2) - 1)) == 0]
    wide = ((top["w"] > top["h"]) & (top["mode"] >= 2) & (top["mode"] < 8)) | ((top["h"] > top["w"]) & (top["mode"] > 60) & (top["mode"] <= 66))
    assert len(top) > 20 and wide.sum() > 0 and (c["ref_idx"] > 0).sum() > 3
    assert changed > 456 * 264 // 2
    check_commands_untouched(uploads, work)

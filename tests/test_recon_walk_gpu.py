"""GPU parity of the RECON pass's command walk (recon_one_ctu, ffvvc_amd/csrc/intra.hip) on hand-built command lists: the walk is
compiled once per wave role, takes its list in windows of 64 commands, adds residuals plainly, joint, scaled or both, and lets
the chroma wave wait for the luma wave on luma_done.  Pictures are one CTU to 2x2 CTUs; every case runs under raster ticket order and
under vvc355_recon_order's, against the oracle's walk of the same lists in decoding order (as tests/test_recon_gpu.py does).

The lists are those a decoder could make: coding units of 8x8 luma samples in z-order, per unit luma PRED, MARK, luma RESID, the
Cb / Cr PREDs (or one CCLM), MARK, the chroma RESIDs — cut off per wave where a case wants an exact command count."""
import ctypes

import numpy as np
import pytest

import bipred_cases as bc
import recon_cases
from conftest import P
from ffvvc_amd import abi, batch

pytestmark = pytest.mark.gpu

C = recon_cases.ReconWork._cmd
ORDERS = ["raster", "critical"]
JOINTS = [1, 3, 5, 7]                 # joint residual: sign and shift, each way


def z_order(n):
    """The cells of an n x n grid (n a power of two) in the order a quadtree visits them."""
    out = []
    for i in range(n * n):
        x = y = 0
        for b in range(8):
            x |= ((i >> (2 * b)) & 1) << b
            y |= ((i >> (2 * b + 1)) & 1) << b
        out.append((x, y))
    return out


def unit_list(work, rng, ox, oy, n_luma=None, n_chroma=None, lmcs=False, first=None, pad=0, cclm_p=0.0, joint_p=0.0):
    """One CTU's list with exactly n_luma commands for the luma wave and n_chroma for the chroma wave (MARKs belong to neither; None:
    all that the CTU's units have).  first: 'cclm' / 'scaled_cb' put a CCLM block / the scaled chroma residuals of a coding unit
    without luma commands at index 0; pad: extra luma RESIDs in the first unit (they move every later command up the list)."""
    ctb, hs, vs = 1 << work.ctb_log2, work.hs, work.vs
    want = [n_luma, n_chroma]
    left = [1 << 30 if n is None else n for n in want]
    out = []

    def take(t, n=1):
        if left[t] < n:
            return False
        left[t] -= n
        return True

    for i, (ux, uy) in enumerate(z_order(ctb // 8)):
        x, y = ox + 8 * ux, oy + 8 * uy
        cu = (x, y, 8, 8)
        cw, chh = 8 >> hs, 8 >> vs
        sc = 8 if lmcs else 0
        marks = [C(abi.RECON_MARK, 0, x, y, 8, 8, *cu), C(abi.RECON_MARK, 1, x, y, 8, 8, *cu)]
        if i == 0 and first == "cclm":
            left[1] -= 1
            out += [C(abi.RECON_CCLM, 1, x, y, 8, 8, *cu, mode=int(rng.choice([81, 82, 83])))] + marks
            continue
        if i == 0 and first == "scaled_cb":
            assert lmcs
            left[1] -= 2
            r = work._resid(1, x, y, cw, chh)
            out += [C(abi.RECON_RESID, 1, x, y, cw, chh, *cu, resid=r, joint=8), C(abi.RECON_RESID, 2, x, y, cw, chh, *cu, resid=r, joint=8 | 1 | 2)] + marks
            continue
        if take(0):
            out.append(C(abi.RECON_PRED, 0, x, y, 8, 8, *cu, mode=int(rng.choice([0, 1, 18, 50] + list(range(2, 67))))))
        out.append(marks[0])
        for _ in range(1 + (pad if i == 0 else 0)):
            if take(0):
                out.append(C(abi.RECON_RESID, 0, x, y, 8, 8, *cu, resid=work._resid(0, x, y, 8, 8)))
        if rng.random() < cclm_p and take(1):
            out.append(C(abi.RECON_CCLM, 1, x, y, 8, 8, *cu, mode=int(rng.choice([81, 82, 83]))))
        else:
            cmode = int(rng.choice([0, 1, 18, 50]))
            for c in (1, 2):
                if take(1):
                    out.append(C(abi.RECON_PRED, c, x, y, 8, 8, *cu, mode=cmode))
        out.append(marks[1])
        if take(1):
            out.append(C(abi.RECON_RESID, 1, x, y, cw, chh, *cu, resid=work._resid(1, x, y, cw, chh), joint=sc))
            if rng.random() < joint_p:
                if take(1):
                    out.append(C(abi.RECON_RESID, 2, x, y, cw, chh, *cu, resid=out[-1][0], joint=sc | int(rng.choice(JOINTS))))
            elif take(1):
                out.append(C(abi.RECON_RESID, 2, x, y, cw, chh, *cu, resid=work._resid(2, x, y, cw, chh), joint=sc))
        if left == [0, 0]:
            break
    assert all(n is None or l == 0 for n, l in zip(want, left)), left
    return out


def hand_work(ncx, ncy, ctb_log2, hs, vs, ctu_list):
    """A ReconWork of ncx x ncy whole CTUs whose lists ctu_list(work, rs, ox, oy) gives.  recon_cases.ReconWork only has a random
    generator for a constructor, so the object is made bare and given what bind(), frame(), _resid() and critical_order() read:
    width, height, ctb_log2, hs, vs, ncx, ncy, slice_idx, col_bd, row_bd, resid_len, tbs, cmds, ctus, order (ciip, ciip_len for
    completeness: no list here has a CIIP command).  A field added to ReconWork that those methods read has to be added here."""
    work = object.__new__(recon_cases.ReconWork)
    ctb = 1 << ctb_log2
    work.width, work.height, work.ctb_log2, work.hs, work.vs = ncx * ctb, ncy * ctb, ctb_log2, hs, vs
    work.ncx, work.ncy = ncx, ncy
    work.slice_idx = np.zeros(ncx * ncy, np.int16)
    work.col_bd = np.array([0] * ncx + [ncx], np.int16)
    work.row_bd = np.array([0] * ncy + [ncy], np.int16)
    work.resid_len, work.tbs, work.ciip, work.ciip_len = 0, [], [], 0
    cmds, ctus = [], np.zeros(ncx * ncy, recon_cases.CTU)
    for rs in range(ncx * ncy):
        lst = ctu_list(work, rs, (rs % ncx) * ctb, (rs // ncx) * ctb)
        ctus[rs]["first_cmd"], ctus[rs]["n_cmd"] = len(cmds), len(lst)
        cmds += lst
    work.cmds = np.array(cmds, recon_cases.CMD)
    work.ctus = ctus
    work.order = np.nonzero(ctus["n_cmd"])[0].astype(np.int32)
    return work


def wave_counts(work, rs):
    """Commands of CTU rs the luma wave / the chroma wave walks."""
    c = work.cmds[work.ctus[rs]["first_cmd"]:][:work.ctus[rs]["n_cmd"]]
    own = c["kind"] != abi.RECON_MARK
    return int((own & (c["c_idx"] == 0)).sum()), int((own & (c["c_idx"] > 0)).sum())


def run_work(dev, orc, work, bd, ticket_order, seed, lmcs=False):
    """The pass on `work` against the oracle, both from the same random picture; returns the number of samples the walk changed."""
    orc.orc_recon_frame_pass.argtypes = [ctypes.c_int, ctypes.POINTER(abi.ReconFrame)]
    orc.orc_recon_frame_pass.restype = None
    rng = np.random.default_rng(seed)
    hs, vs, w, h = work.hs, work.vs, work.width, work.height
    isz = 1 if bd == 8 else 2
    raster = np.nonzero(work.ctus["n_cmd"])[0].astype(np.int32)
    work.order = recon_cases.critical_order(dev, work.ctus, work.ncx, work.ncy) if ticket_order == "critical" else raster
    assert sorted(work.order.tolist()) == raster.tolist()
    model = recon_cases.ReconWork.lmcs_model(np.random.default_rng(0x1A5C + bd), bd) if lmcs else None
    d_model = batch.DeviceBuffer.from_host(np.frombuffer(bytes(model), np.uint8)) if lmcs else None
    dims = [(w, h), (w >> hs, h >> vs), (w >> hs, h >> vs)]
    planes = [bc.smooth_picture(rng, ph, pw, bd, scale=16) for (pw, ph) in dims]
    resid = rng.integers(-(1 << (bd - 3)), 1 << (bd - 3), size=max(1, work.resid_len)).astype(np.int32)
    want = [p.copy() for p in planes]
    hc = work.bind(resid.ctypes.data, 0, isz)
    hf = work.frame([P(p) for p in want], [d[0] * isz for d in dims], hc.ctypes.data, work.ctus.ctypes.data, raster.ctypes.data, 0,
                    work.slice_idx.ctypes.data, work.col_bd.ctypes.data, work.row_bd.ctypes.data, collocated=int(rng.integers(0, 2)),
                    lmcs_ptr=ctypes.addressof(model) if lmcs else 0)
    orc.orc_recon_frame_pass(bd, ctypes.byref(hf))
    pitched = [batch.to_pitched(p) for p in planes]
    d_planes = [batch.DeviceBuffer.from_host(p) for p in pitched]
    d_res = batch.DeviceBuffer.from_host(resid)
    dcmd = work.bind(d_res.ptr, 0, isz)
    # the pad bytes are the pass's own: whatever the host leaves there must not matter
    dcmd.view(np.uint8).reshape(len(dcmd), -1)[:, 34:40] = np.random.default_rng(len(dcmd)).integers(0, 256, size=(len(dcmd), 6), dtype=np.uint8)
    d_cmds, d_ctus, d_order = batch.DeviceBuffer.from_host(dcmd.view(np.uint8)), batch.DeviceBuffer.from_host(work.ctus.view(np.uint8)), batch.DeviceBuffer.from_host(work.order)
    d_state = batch.DeviceBuffer(dev.vvc355_recon_state_bytes(work.ncx * work.ncy))
    d_slice, d_col, d_row = batch.DeviceBuffer.from_host(work.slice_idx), batch.DeviceBuffer.from_host(work.col_bd), batch.DeviceBuffer.from_host(work.row_bd)
    df = work.frame([b.ptr for b in d_planes], [p.shape[1] * isz for p in pitched], d_cmds.ptr, d_ctus.ptr, d_order.ptr, d_state.ptr,
                    d_slice.ptr, d_col.ptr, d_row.ptr, collocated=hf.collocated, lmcs_ptr=d_model.ptr if lmcs else 0)
    d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(df), np.uint8))
    for rep in range(2):           # the second pass starts from the first one's pad bytes and scheduling state
        for b, p in zip(d_planes, pitched):
            dev.vvc355_upload(b.ptr, p.ctypes.data, p.nbytes)
        dev.vvc355_recon_frame_pass(None, bd, d_f.ptr, ctypes.addressof(df))
        dev.vvc355_stream_sync(None)
        for c in range(3):
            got = d_planes[c].to_host(pitched[c].dtype, pitched[c].shape)[:, :dims[c][0]]
            bad = np.argwhere(got != want[c])
            assert len(bad) == 0, (f"pass {rep} bd={bd} {w}x{h} ctb={1 << work.ctb_log2} component {c}: {len(bad)} samples differ, first at (y, x) = "
                                   f"{bad[0].tolist()}; {len(work.cmds)} commands in {len(work.order)} CTUs")
    return sum(int((want[c] != planes[c]).sum()) for c in range(3))


def full_lists(rng, **kw):
    """Every coding unit of every CTU, all its commands."""
    return lambda work, rs, ox, oy: unit_list(work, rng, ox, oy, **kw)


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("ctb_log2", [5, 6, 7])
def test_walk_ctb_sizes_and_depths_tile_path(dev, orc, ctb_log2, bd, ticket_order):
    """4:2:0, 2x2 CTUs of 32 / 64 / 128 at 8 / 10 / 12 bits: both roles' copies of the walk on LDS tiles with every command kind they keep —
    twins, CCLM, plain, joint and scaled residuals (chroma residual scaling on)."""
    rng = np.random.default_rng(0x3A1C0000 + 16 * ctb_log2 + bd)
    work = hand_work(2, 2, ctb_log2, 1, 1, full_lists(rng, lmcs=True, cclm_p=0.25, joint_p=0.3))
    k = work.cmds["kind"]
    assert (k == abi.RECON_CCLM).sum() > 3 and ((work.cmds["joint"] & 9) == 9).sum() > 3
    changed = run_work(dev, orc, work, bd, ticket_order, 0x3A1C1000 + 16 * ctb_log2 + bd, lmcs=True)
    assert changed > work.width * work.height // 2


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("bd,fmt,ctb_log2", [(10, (1, 0), 6), (12, (0, 0), 5)])
def test_walk_plane_path(dev, orc, bd, fmt, ctb_log2, ticket_order):
    """One 4:2:2 and one 4:4:4 picture: the same walk on the planes in device memory."""
    rng = np.random.default_rng(0x3A1C2000 + bd)
    work = hand_work(2, 2, ctb_log2, *fmt, full_lists(rng, lmcs=True, cclm_p=0.25, joint_p=0.3))
    changed = run_work(dev, orc, work, bd, ticket_order, 0x3A1C2100 + bd, lmcs=True)
    assert changed > work.width * work.height // 2


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_walk_command_counts_at_window_edges(dev, orc, n, ticket_order):
    """n commands for each wave in every CTU (128x128 CTUs, 2x2): a wave's list ends just before, at and just after a window of 64
    list entries hands over to the next."""
    rng = np.random.default_rng(0x3A1C3000 + n)
    work = hand_work(2, 2, 7, 1, 1, lambda wk, rs, ox, oy: unit_list(wk, rng, ox, oy, n, n, lmcs=True, joint_p=0.3))
    for rs in range(4):
        assert wave_counts(work, rs) == (n, n)
    run_work(dev, orc, work, 10, ticket_order, 0x3A1C3100 + n, lmcs=True)


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_walk_list_lengths_at_window_edges(dev, orc, n, ticket_order):
    """One CTU whose whole list is n luma commands (no MARK, no chroma command): the list itself, not only a wave's share of it, ends
    at the window's edge."""
    rng = np.random.default_rng(0x3A1C3800 + n)
    work = hand_work(1, 1, 7, 1, 1, lambda wk, rs, ox, oy: [c for c in unit_list(wk, rng, ox, oy, n, 0) if c[10] != abi.RECON_MARK])
    assert work.ctus["n_cmd"][0] == n and wave_counts(work, 0) == (n, 0)
    assert run_work(dev, orc, work, 10, ticket_order, 0x3A1C3900 + n) > 0


@pytest.mark.parametrize("ticket_order", ORDERS)
def test_walk_twin_across_windows(dev, orc, ticket_order):
    """A Cb PRED at list index 63 whose twin Cr PRED is index 64, the first command of the next window: the pair cannot go through one
    pass (the planner sees one window), each is predicted on its own."""
    rng = np.random.default_rng(0x3A1C4000)
    work = hand_work(2, 2, 6, 1, 1, lambda wk, rs, ox, oy: unit_list(wk, rng, ox, oy, 128 + 4, 256, pad=4))
    for rs in range(4):
        c = work.cmds[work.ctus[rs]["first_cmd"]:]
        assert (c["kind"][63], c["c_idx"][63], c["kind"][64], c["c_idx"][64]) == (abi.RECON_PRED, 1, abi.RECON_PRED, 2) and c["mode"][63] == c["mode"][64]
        assert (c["kind"][7], c["c_idx"][7], c["kind"][8], c["c_idx"][8]) == (abi.RECON_PRED, 1, abi.RECON_PRED, 2)         # ... and twins inside a window
    run_work(dev, orc, work, 10, ticket_order, 0x3A1C4100)


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("role", [0, 1])
def test_walk_last_windows_of_one_role(dev, orc, role, ticket_order):
    """The other wave's commands end in the first window: every later window holds commands of one role only (and MARKs)."""
    rng = np.random.default_rng(0x3A1C5000 + role)
    n = [(128, 6), (3, 256)][role]
    work = hand_work(2, 2, 6, 1, 1, lambda wk, rs, ox, oy: unit_list(wk, rng, ox, oy, *n, lmcs=True))
    for rs in range(4):
        c = work.cmds[work.ctus[rs]["first_cmd"]:][:work.ctus[rs]["n_cmd"]][64:]
        own = c[c["kind"] != abi.RECON_MARK]
        assert len(c) > 64 and len(own) > 32 and ((own["c_idx"] > 0) == (role == 1)).all()
    run_work(dev, orc, work, 10, ticket_order, 0x3A1C5100 + role, lmcs=True)


def resid_gallery(work, rng, ox, oy):
    """Residual adds only: luma blocks 1 to 128 wide, then chroma blocks 1 to 64 wide in every variant — plain, joint with both signs
    and shifts, scaled, joint and scaled — two of them of 2048 samples (more than the 1024 a command's prefetch covers).  RESIDs
    follow each other, so every second one comes prefetched and the one behind it does not; the first of a window never does.  All
    luma commands come first: the scaled blocks read the luma around their 64x64 units."""
    out = [C(abi.RECON_MARK, t, ox, oy, 128, 128, ox, oy, 128, 128) for t in (0, 1)]
    for i, (w, h) in enumerate([(1, 8), (2, 8), (4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (128, 8), (1, 16), (64, 16)]):
        x = ox + (3 + 8 * i if w < 4 else 4 * int(rng.integers(0, (128 - w) // 4 + 1)))          # the narrow ones at odd columns
        y = oy + 4 * int(rng.integers(0, (128 - h) // 4 + 1))
        out.append(C(abi.RECON_RESID, 0, x, y, w, h, ox, oy, 128, 128, resid=work._resid(0, x, y, w, h)))
    i = 0
    for w, h in [(1, 8), (2, 8), (4, 4), (8, 4), (16, 8), (32, 64), (64, 32)]:
        for joint in [0] + JOINTS + [8] + [8 | j for j in JOINTS]:
            xc = 1 + 2 * int(rng.integers(0, 30)) if w < 4 else 4 * int(rng.integers(0, (64 - w) // 4 + 1))
            yc = 4 * int(rng.integers(0, (64 - h) // 4 + 1))
            cu = (ox + 64 * (i & 1), oy + 64 * ((i >> 1) & 1), 64, 64)          # the 64x64 unit whose scale the block takes
            out.append(C(abi.RECON_RESID, 2 if i % 3 == 0 else 1, ox + 2 * xc, oy + 2 * yc, w, h, *cu, resid=work._resid(1, xc, yc, w, h), joint=joint))
            i += 1
    return out


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("bd", [8, 10])
def test_walk_resid_variants(dev, orc, bd, ticket_order):
    """Every residual-add variant at every width (resid_gallery), in 2x2 CTUs of 128x128."""
    rng = np.random.default_rng(0x3A1C6000 + bd)
    work = hand_work(2, 2, 7, 1, 1, lambda wk, rs, ox, oy: resid_gallery(wk, rng, ox, oy))
    res = work.cmds[work.cmds["kind"] == abi.RECON_RESID]
    assert sorted(set(res["w"].tolist())) == [1, 2, 4, 8, 16, 32, 64, 128] and (res["w"].astype(int) * res["h"] > 1024).sum() >= 12
    assert sorted(set(res["joint"].tolist())) == sorted([0] + JOINTS + [8] + [8 | j for j in JOINTS]) and work.ctus["n_cmd"][0] > 64
    assert run_work(dev, orc, work, bd, ticket_order, 0x3A1C6100 + bd, lmcs=True) > 0


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("first", ["scaled_cb", "cclm"])
def test_walk_command_0_reads_luma(dev, orc, first, ticket_order):
    """Command 0 of every CTU is a scaled Cb RESID (an inter coding unit with chroma residuals only: itransform runs before
    add_reconstructed_area) or a CCLM block over luma the walk does not write: the chroma wave needs the luma apron / the luma tile
    before any luma command is done, so it must wait until the luma wave has loaded its edges (luma_done starts at -1)."""
    rng = np.random.default_rng(0x3A1C7000 + len(first))
    work = hand_work(2, 2, 6, 1, 1, full_lists(rng, lmcs=True, first=first, cclm_p=0.2, joint_p=0.2))
    for rs in range(4):
        c = work.cmds[work.ctus[rs]["first_cmd"]]
        assert (c["kind"], c["c_idx"]) == ((abi.RECON_RESID, 1) if first == "scaled_cb" else (abi.RECON_CCLM, 1)) and (first == "cclm" or c["joint"] == 8)
    run_work(dev, orc, work, 10, ticket_order, 0x3A1C7100 + len(first), lmcs=True)


@pytest.mark.parametrize("ticket_order", ORDERS)
@pytest.mark.parametrize("role", [0, 1])
def test_walk_ctu_without_commands_of_one_role(dev, orc, role, ticket_order):
    """CTUs with no luma command at all (role 0) / no chroma command at all (role 1) next to ordinary ones: that wave waits, loads,
    publishes and joins without walking anything, and its neighbours still find its flags."""
    rng = np.random.default_rng(0x3A1C8000 + role)

    def ctu_list(wk, rs, ox, oy):
        if rs in (0, 3):
            return full_lists(rng, lmcs=True, cclm_p=0.2)(wk, rs, ox, oy)
        return unit_list(wk, rng, ox, oy, 0 if role == 0 else 128, 256 if role == 0 else 0, lmcs=True)
    work = hand_work(2, 2, 6, 1, 1, ctu_list)
    assert wave_counts(work, 1)[role] == 0 and wave_counts(work, 2)[role] == 0 and min(wave_counts(work, 0)) > 0
    run_work(dev, orc, work, 10, ticket_order, 0x3A1C8100 + role, lmcs=True)

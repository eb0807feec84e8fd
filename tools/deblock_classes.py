#!/usr/bin/env python3
"""Which filter class does every deblocking segment of the bench's picture decide on, and how much of a wave idles because its lanes
decided differently?

    python tools/deblock_classes.py [--width W --height H --bd BD] OUT.json

Builds the bench's own first picture (bench.Frame with its seed, bench.build_chain), runs the chain up to the deblocking passes on
the device, copies the planes and the side tables each pass reads to the host, and restates the decisions of
ff_vvc_deblock_vertical / _horizontal (vvc_filter.c:864-1003, vvc_filter_template.c:466-804, h2656_deblock_template.c:25-99) in
numpy: nothing here runs inside a kernel.  Per pass and component: segments per class (bs == 0; no filter: tc == 0 or the decision
says so; weak by samples changed per side; strong; long by (len_p, len_q)).  For luma also the lanes of deblock_frame_kernel in their
launch order, compacted per workgroup as the kernel's phase A does it, and per wave the filter bodies that some lane needs: the
share of (wave, body) lane-slots whose lane is masked off."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ffvvc_amd import abi  # noqa: E402


def table(lib, name, ctype, n):
    return np.array((ctype * n).in_dll(lib, name), np.int64)


def download(lib, dev_ptr, shape, dtype):
    out = np.empty(shape, dtype)
    lib.vvc355_download(out.ctypes.data, dev_ptr, out.nbytes)
    return out


def d2(a, b, c):
    return np.abs(a - 2 * b + c)


def taps(A, lines_rows, n_units, pos_of_unit):
    """p[i], q[i] (i < 8) of the given rows for an edge at every position in pos_of_unit (samples across; A padded by 8 on both sides)."""
    R = np.pad(A[lines_rows].astype(np.int64), ((0, 0), (8, 8)))
    p = [R[:, 8 + pos_of_unit - 1 - i] for i in range(8)]
    q = [R[:, 8 + pos_of_unit + i] for i in range(8)]
    return p, q


def luma_pass(A, T, f, bd, tcT, betaT, vertical):
    """A: luma plane with the edges running down the columns (the horizontal pass transposed); T: the pass's tables, oriented alike.
    Returns the class of every segment [4-line group along, 4-sample unit across] as strings' indices, and the names."""
    ua, ue = A.shape[0] // 4, A.shape[1] // 4
    pos = np.arange(ue) * 4
    P0, Q0 = taps(A, slice(0, None, 4), ue, pos)
    P3, Q3 = taps(A, slice(3, None, 4), ue, pos)
    P0, Q0, P3, Q3 = ([t[:ua] for t in s] for s in (P0, Q0, P3, Q3))
    bs, lp, lq = T["bs"][:ua, :ue].astype(np.int64), T["len_p"][:ua, :ue].astype(np.int64), T["len_q"][:ua, :ue].astype(np.int64)
    r, k = np.meshgrid(np.arange(ua), np.arange(ue), indexing="ij")
    qpo = T["qp_y"].astype(np.int64)
    qp = (qpo[np.minimum(r // 2, qpo.shape[0] - 1), np.maximum(4 * k - 1, 0) // 8] + qpo[np.minimum(r // 2, qpo.shape[0] - 1), np.minimum(k // 2, qpo.shape[1] - 1)] + 1) >> 1
    if f.ladf_enabled:
        level = (P0[0] + P3[0] + Q0[0] + Q3[0]) >> 2
        off = np.full_like(level, f.ladf_lowest_qp_offset)
        go = np.ones(level.shape, bool)
        for i in range(4):
            go &= (i < f.num_ladf_intervals - 1) & (level > f.ladf_lower_bound[i + 1])
            off = np.where(go, f.ladf_qp_offset[i], off)
        qp = qp + off
    beta = betaT[np.clip(qp + T["beta_off"][:ua, :ue], 0, 63)] << (bd - 8)
    tc_in = tcT[np.clip(qp + 2 * (bs - 1) + (T["tc_off"][:ua, :ue] & -2), 0, 65)]
    tc = (tc_in + (1 << (9 - bd))) >> (10 - bd) if bd < 10 else tc_in << (bd - 10)
    hce = T["hor_ctu_edge"][None, :ue] if not vertical else np.zeros((1, ue), bool)
    dp0, dq0, dp3, dq3 = d2(P0[2], P0[1], P0[0]), d2(Q0[2], Q0[1], Q0[0]), d2(P3[2], P3[1], P3[0]), d2(Q3[2], Q3[1], Q3[0])
    d0, d3 = dp0 + dq0, dp3 + dq3
    tc25 = (tc * 5 + 1) >> 1
    large_p, large_q = (lp > 3) & ~hce, lq > 3
    large = large_p | large_q
    LP, LQ = np.where(large_p, lp, 3), np.where(large_q, lq, 3)

    def side(P, L, big, dbase):
        dl = np.where(big, (dbase + d2(P[5], P[4], P[3]) + 1) >> 1, dbase)
        sl = np.abs(P[3] - P[0]) + np.where(L == 7, np.abs(P[7] - P[6] - P[5] + P[4]), 0)
        at = np.where(L == 7, P[7], np.where(L == 5, P[5], P[3]))
        return dl, np.where(big, (sl + np.abs(P[3] - at) + 1) >> 1, sl)

    dp0l, sp0 = side(P0, LP, large_p, dp0)
    dq0l, sq0 = side(Q0, LQ, large_q, dq0)
    dp3l, sp3 = side(P3, LP, large_p, dp3)
    dq3l, sq3 = side(Q3, LQ, large_q, dq3)
    d0l, d3l = dp0l + dq0l, dp3l + dq3l
    beta53, beta_4 = (beta * 3) >> 5, beta >> 4
    apq0, apq3 = np.abs(P0[0] - Q0[0]), np.abs(P3[0] - Q3[0])
    is_long = large & (d0l + d3l < beta) & (sp0 + sq0 < beta53) & (apq0 < tc25) & (sp3 + sq3 < beta53) & (apq3 < tc25) & ((d0l << 1) < beta_4) & ((d3l << 1) < beta_4)
    lp_e, lq_e = np.where(large, LP, lp), np.where(large, LQ, lq)                 # the large branch overwrites the lengths it was given
    beta_3, beta_2 = beta >> 3, beta >> 2
    strong = ((lp_e > 2) & (lq_e > 2) & (np.abs(P0[3] - P0[0]) + np.abs(Q0[3] - Q0[0]) < beta_3) & (apq0 < tc25)
              & (np.abs(P3[3] - P3[0]) + np.abs(Q3[3] - Q3[0]) < beta_3) & (apq3 < tc25) & ((d0 << 1) < beta_2) & ((d3 << 1) < beta_2))
    side_lim = (beta + (beta >> 1)) >> 3
    two = (lp_e > 1) & (lq_e > 1)
    nd_p, nd_q = np.where(two & (dp0 + dp3 < side_lim), 2, 1), np.where(two & (dq0 + dq3 < side_lim), 2, 1)
    names = ["bs0", "no_filter", "strong"] + [f"weak_{a}_{b}" for a in (1, 2) for b in (1, 2)] + [f"long_{a}_{b}" for a in (3, 5, 7) for b in (3, 5, 7)]
    cls = np.full((ua, ue), 1, np.int64)
    weak = (d0 + d3 < beta)
    cls = np.where(weak, 3 + (nd_p - 1) * 2 + (nd_q - 1), cls)
    cls = np.where(weak & strong, 2, cls)
    n3 = lambda L: np.where(L == 3, 0, np.where(L == 5, 1, 2))
    cls = np.where(is_long, 7 + n3(LP) * 3 + n3(LQ), cls)
    cls = np.where(tc == 0, 1, cls)
    cls = np.where(bs == 0, 0, cls)
    cls[:, 0] = 0                                                              # no edge at the picture's border
    return cls, names


def chroma_pass(A, T, c, f, bd, tcT, betaT, vertical, sa, sl):
    """A: a chroma plane, oriented as in luma_pass; sa / sl: its subsampling across / along the edges."""
    lines = 4 >> sl
    ua, ue = T["bs_c"][c - 1].shape
    ua = min(ua, A.shape[0] // lines)
    k_units = np.arange(ue)
    pos = (k_units * 4) >> sa
    P0, Q0 = taps(A, slice(0, None, lines), ue, pos)
    P1, Q1 = taps(A, slice(lines - 1, None, lines), ue, pos)
    P0, Q0, P1, Q1 = ([t[:ua] for t in s] for s in (P0, Q0, P1, Q1))
    bs = T["bs_c"][c - 1][:ua].astype(np.int64)
    on_grid = ((k_units * 4) % (8 << sa) == 0) & (k_units > 0)
    km1 = np.maximum(k_units - 1, 0)
    qc = T["qp_c"][c - 1][:ua].astype(np.int64)
    qp = (qc[:, km1] + qc - 2 * f.qp_bd_offset + 1) >> 1
    tbs = T["tb_c"][:ua].astype(np.int64)
    big = (tbs[:, km1] >= 8) & (tbs >= 8)
    hce = T["hor_ctu_edge"][None, :ue] if not vertical else np.zeros((1, ue), bool)
    len_q = np.where(big, 3, (bs == 2).astype(np.int64))
    len_p = np.where(big, np.where(hce, 1, 3), (bs == 2).astype(np.int64))
    beta = betaT[np.clip(qp + T["beta_off_c"][c - 1][:ua], 0, 63)] << (bd - 8)
    tc_in = tcT[np.clip(qp + 2 * (bs - 1) + (T["tc_off_c"][c - 1][:ua] & -2), 0, 65)]
    tc = (tc_in + (1 << (9 - bd))) >> (10 - bd) if bd < 10 else tc_in << (bd - 10)
    one = len_p == 1
    beta_3, beta_2, tc25 = beta >> 3, beta >> 2, (tc * 5 + 1) >> 1

    def line(P, Q):
        p2, p3 = np.where(one, P[1], P[2]), np.where(one, P[1], P[3])
        dd = d2(p2, P[1], P[0]) + d2(Q[2], Q[1], Q[0])
        ok = ((dd << 1) < beta_2) & (np.abs(p3 - P[0]) + np.abs(Q[0] - Q[3]) < beta_3) & (np.abs(P[0] - Q[0]) < tc25)
        return dd, ok

    dd0, ok0 = line(P0, Q0)
    dd1, ok1 = line(P1, Q1)
    strong = (len_q == 3) & (dd0 + dd1 < beta) & ok0 & ok1
    names = ["bs0", "no_filter", "weak_1_1", "strong_1_3", "strong_3_3"]
    cls = np.where(strong, np.where(len_p == 3, 4, 3), 2)
    cls = np.where((tc == 0) | (len_p == 0) | (len_q == 0), 1, cls)
    cls = np.where((bs == 0) | ~on_grid[None, :], 0, cls)
    return cls[:, on_grid], names


def lane_slots(cls, vertical, names):
    """deblock_frame_kernel's luma lanes in launch order, the lanes with bs != 0 compacted per workgroup of 256, waves of 64."""
    ua, ue = cls.shape
    ua2 = (ua + 1) // 2 * 2
    c = np.zeros((ua2, ue), np.int64)
    c[:ua] = cls
    c = c[:, 1:]                                                               # edges 1 .. ue - 1
    ne, na = ue - 1, ua2 // 2
    if vertical:                                                               # unit = ku * n_edges + ke, lane = 2 * unit + seg
        flat = c.reshape(na, 2, ne).transpose(0, 2, 1).reshape(-1)
    else:                                                                      # unit = ke * n_along + ku
        flat = c.T.reshape(-1)
    body = np.full(len(names), -1)
    for i, n in enumerate(names):
        body[i] = 0 if n.startswith("weak") else 1 if n == "strong" else 2 if n.startswith("long") else -1
    wg = np.arange(flat.size) // 256
    active = flat > 0
    rank = np.cumsum(active) - 1
    start =np.r_[0, np.cumsum(np.bincount(wg, weights=active).astype(np.int64))[:-1]]
    wave = wg * 4 + (rank - start[wg]) // 64
    wave, kind, fine = wave[active], body[flat[active]], flat[active]
    filt = kind >= 0
    out = {"lanes": int(flat.size), "lanes_with_bs": int(active.sum()), "waves_after_compaction": int(np.unique(wave).size),
           "lanes_that_filter": int(filt.sum()), "waves_with_no_filtering_lane": int(np.unique(wave).size - np.unique(wave[filt]).size)}
    for label, key in (("three_bodies_weak_strong_long", kind), ("fine_classes", fine)):
        pairs = np.unique(np.stack([wave[filt], key[filt]]), axis=1).shape[1]
        out[label] = {"wave_body_pairs": int(pairs), "lane_slots": int(pairs * 64), "masked_off_share": round(float(1 - filt.sum() / (pairs * 64)), 4) if pairs else None}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bd", type=int, default=10)
    args = ap.parse_args()
    import torch
    lib = abi.load()
    lib.vvc355_set_device(0)
    frame = bench.Frame(torch, args.width, args.height, args.bd, seed=0x5EED0001)
    frame.noise = False
    chain = bench.build_chain(lib, torch, frame)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):                                                         # the picture as the bench's timed steps see it: not the first pass
        for st in chain:
            st.launch(stream)
    torch.cuda.synchronize()
    raw = ctypes.CDLL(abi.LIB_PATH)
    tcT, betaT = table(raw, "vvc355_tab_tc_table", ctypes.c_uint16, 66), table(raw, "vvc355_tab_beta_table", ctypes.c_uint8, 64)
    frames = {int(f.vertical): f for f in frame.keep if isinstance(f, abi.DeblockFrame)}
    w, h, bd = args.width, args.height, args.bd
    tw, th = w // 4, h // 4
    res = {"picture": f"{w}x{h} {bd}-bit, bench.Frame seed 0x5EED0001 (the first picture of --gop 0)", "passes": {}}
    for st in chain:
        if st.name in ("deblock_vertical", "deblock_horizontal"):
            vertical = st.name == "deblock_vertical"
            torch.cuda.synchronize()
            f = frames[int(vertical)]
            planes = [t.cpu().numpy() for t in st.writes]
            dims = [(w, h), (w >> f.hs, h >> f.vs), (w >> f.hs, h >> f.vs)]
            planes = [p[:dims[c][1], :dims[c][0]] for c, p in enumerate(planes)]
            o = (lambda a: a) if vertical else (lambda a: np.ascontiguousarray(a.T))
            ctb = (np.arange(tw)[None, :] * 4 >> f.ctb_log2) + (np.arange(th)[:, None] * 4 >> f.ctb_log2) * f.ctb_width
            dbp = download(lib, f.db_params, (ctb.max() + 1, 6), np.int8).astype(np.int64)
            T = {"bs": o(download(lib, f.bs[0], (th, tw), np.uint8)), "len_p": o(download(lib, f.max_len_p, (th, tw), np.uint8)),
                 "len_q": o(download(lib, f.max_len_q, (th, tw), np.uint8)), "qp_y": o(download(lib, f.qp_y, (h // 8, w // 8), np.int8)),
                 "beta_off": o(dbp[ctb, 0]), "tc_off": o(dbp[ctb, 3]),
                 "bs_c": [o(download(lib, f.bs[c], (th, tw), np.uint8)) for c in (1, 2)], "qp_c": [o(download(lib, f.qp_c[c], (th, tw), np.int8)) for c in (0, 1)],
                 "tb_c": o(download(lib, f.tb_size_c, (th, tw), np.uint8)),
                 "beta_off_c": [o(dbp[ctb, c]) for c in (1, 2)], "tc_off_c": [o(dbp[ctb, 3 + c]) for c in (1, 2)],
                 "hor_ctu_edge": (np.arange(th) * 4) % (1 << f.ctb_log2) == 0}
            entry = {}
            cls, names = luma_pass(o(planes[0]), T, f, bd, tcT, betaT, vertical)
            n = np.bincount(cls[:, 1:].ravel(), minlength=len(names))
            entry["luma"] = {"segments": {nm: int(v) for nm, v in zip(names, n) if v}, "lanes": lane_slots(cls, vertical, names)}
            sa, sl = (f.hs, f.vs) if vertical else (f.vs, f.hs)
            for c in (1, 2):
                cc, cn = chroma_pass(o(planes[c]), T, c, f, bd, tcT, betaT, vertical, sa, sl)
                n = np.bincount(cc.ravel(), minlength=len(cn))
                entry["Cb" if c == 1 else "Cr"] = {"segments": {nm: int(v) for nm, v in zip(cn, n) if v}}
            before = planes[0].copy()
            st.launch(stream)
            torch.cuda.synchronize()
            after = st.writes[0].cpu().numpy()[:h, :w]
            # cross-check of the restatement against what the device did (the bench verifies that against the oracle): every luma
            # sample the pass changed lies within the taps that the class of its segment may change
            ch = o(before != after)
            ua, ue = cls.shape
            reach = {i: ((3, 3) if nm == "strong" else tuple(int(v) for v in nm.split("_")[1:])) for i, nm in enumerate(names) if i >= 2}
            allowed = np.zeros((ua, ue * 4 + 16), bool)
            for i, (n_p, n_q) in reach.items():
                rr, kk = np.nonzero(cls == i)
                for d in range(-n_p, n_q):
                    allowed[rr, 8 + kk * 4 + d] = True
            allowed = np.repeat(allowed[:, 8:8 + ch.shape[1]], 4, axis=0)[:ch.shape[0]]
            entry["luma"]["changed_luma_sample_fraction"] = round(float(ch.mean()), 4)
            entry["luma"]["changed_samples_outside_their_class"] = int((ch[:allowed.shape[0]] & ~allowed).sum())
            res["passes"][st.name] = entry
        else:
            st.launch(stream)
    torch.cuda.synchronize()
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()

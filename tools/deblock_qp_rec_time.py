"""What vvc355_deblock_qp_rec_pass saves a caller of the record path, on two pictures: bs_rec_cases.BIG (1480x840, CTU 128) and an 8K tiling
of it (7680x4320: the picture's records repeated every 1536 x 896 samples, 5 x 5 times, the records that end below the picture dropped;
the gaps between the tiles stay uncovered and come out as zeros).  Three groups of numbers per picture:
  bytes    what a caller uploads: the three QP planes against the two sidecars.  Computed from the record counts, not measured.
  h2d      (a) the pinned host-to-device copy of the three planes, against (b) the copy of the two sidecars + the kernel, each between
           device events of its own, alternating, medians.
  kernel   vvc355_deblock_qp_rec_pass alone, next to vvc355_deblock_bs_rec_pass on the same records, alternating in the same loop.
The device's tables must equal the numpy painter's (qp_rec_cases.expected) before anything is timed.  A tool, not a test: it needs an
MI355X and fails without one; it reads nothing outside the repository.

    python tools/deblock_qp_rec_time.py [--reps 100] [--rounds 5] [--out profiles/deblock_qp_rec_pass.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE_W, TILE_H = 1536, 896                    # BIG rounded up to whole CTUs


def clock_state():
    """The clocks as the driver reports them (read only), before and after the timed loops."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, timeout=60, text=True)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr[-200:]}
    except Exception as e:                    # no tool, no permission: say so in the profile instead of failing the measurement
        return {"unavailable": repr(e)}


def tiled(t, recs, width, height):
    """The record arrays of `t` repeated every TILE_W x TILE_H samples over width x height; records that end outside are dropped."""
    out = []
    for r in recs:
        parts = []
        for ty in range((height + TILE_H - 1) // TILE_H):
            for tx in range(width // TILE_W):
                c = r.copy()
                c["x0"] += tx * TILE_W
                c["y0"] += ty * TILE_H
                parts.append(c[c["y0"].astype(np.int64) + c["h"] <= height])
        out.append(np.concatenate(parts))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every piece (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deblock_qp_rec_pass.json"))
    args = ap.parse_args()

    import torch
    import bs_cases
    import bs_rec_cases as rc
    import qp_rec_cases as qc
    from ffvvc_amd import abi
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("deblock_qp_rec_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    big = bs_cases.BsTables(np.random.default_rng(rc.SEED + len(rc.CASES)), **rc.BIG)

    def measure(label, width, height, recs):
        g = qc.geometry(width, height, 7)
        t = SimpleNamespace(**vars(g), hs=big.hs, vs=big.vs, lfase=1, lfate=1)
        n_ctb, n_units = g.cw * g.ch, g.tw * g.th
        (cu, cu_first), (tu, tu_first), (mv, mv_first) = [bs_cases.BsTables.group_per_ctu(r, 7, g.cw, n_ctb) for r in recs]
        cu_qp, tu_qp_c = qc.sidecars(np.random.default_rng(qc.SEED + 400), len(cu), len(tu))
        p = qc.Pic(g=g, cu=cu, tu=tu, cu_first=cu_first, tu_first=tu_first, cu_qp=cu_qp, tu_qp_c=tu_qp_c)
        want = qc.expected(p)

        def on_device(a):
            return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

        d_cu, d_cu_first, d_tu, d_tu_first, d_mv, d_mv_first = (on_device(a) for a in (cu, cu_first, tu, tu_first, mv, mv_first))
        small = {"ref_poc": big.ref_poc, "slice_idx": np.zeros(n_ctb, np.int16), "col_bd": np.zeros(g.cw + 1, np.int16), "row_bd": np.zeros(g.ch + 1, np.int16)}
        tabs = {k: on_device(v) for k, v in small.items()}
        tabs["mvf"] = torch.zeros(n_units * 24, dtype=torch.uint8, device="cuda")
        for name in big.OUT + rc.TB_C + qc.TABLES:
            tabs[name] = torch.full((n_units,), 0xEE, dtype=torch.uint8, device="cuda")
        # pinned host copies and their device destinations: (a) the planes a caller paints on the host, (b) the sidecars
        h_planes = [torch.from_numpy(want[n].view(np.uint8).reshape(-1).copy()).pin_memory() for n in qc.TABLES]
        d_upload = [torch.empty(h.numel(), dtype=torch.uint8, device="cuda") for h in h_planes]
        h_side = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).pin_memory() for a in (cu_qp, tu_qp_c)]
        d_side = [torch.empty(h.numel(), dtype=torch.uint8, device="cuda") for h in h_side]
        for d, h in zip(d_side, h_side):
            d.copy_(h)

        fill = bs_cases.BsTables.fill_frame(t, 0, 0, d_mv.data_ptr(), (0, 0, len(mv)), lambda name: tabs["mvf"].data_ptr() if name == "mvf" else 0,
                                            (0, 0, d_mv_first.data_ptr()))
        bsf = rc.rec_frame(t, (d_cu.data_ptr(), len(cu), d_cu_first.data_ptr()), (d_tu.data_ptr(), len(tu), d_tu_first.data_ptr()),
                           lambda name: tabs[name].data_ptr())
        qpf = qc.qp_frame(g, (d_cu.data_ptr(), len(cu), d_cu_first.data_ptr()), (d_tu.data_ptr(), len(tu), d_tu_first.data_ptr()),
                          d_side[0].data_ptr(), d_side[1].data_ptr(), [tabs[n].data_ptr() for n in qc.TABLES], g.tw)
        d_fill, d_bsf, d_qpf = (on_device(np.frombuffer(bytes(f), np.uint8)) for f in (fill, bsf, qpf))
        dev.vvc355_tab_fill_pass(st, d_fill.data_ptr(), ctypes.addressof(fill))

        def bs_pass():
            assert dev.vvc355_deblock_bs_rec_pass(st, d_bsf.data_ptr(), ctypes.addressof(bsf)) == 0

        def qp_pass():
            assert dev.vvc355_deblock_qp_rec_pass(st, d_qpf.data_ptr(), ctypes.addressof(qpf)) == 0

        def planes_h2d():
            for d, h in zip(d_upload, h_planes):
                d.copy_(h, non_blocking=True)

        def sidecars_h2d_and_kernel():
            for d, h in zip(d_side, h_side):
                d.copy_(h, non_blocking=True)
            qp_pass()

        pieces = {"bs_rec_kernel": bs_pass, "qp_rec_kernel": qp_pass, "a_planes_h2d": planes_h2d, "b_sidecars_h2d_and_kernel": sidecars_h2d_and_kernel}
        # the device's tables against the painter's first (this also warms every piece once)
        for launch in pieces.values():
            launch()
        torch.cuda.synchronize()
        differing = [n for n in qc.TABLES if not np.array_equal(tabs[n].cpu().numpy().view(np.int8).reshape(g.th, g.tw), want[n])]
        for _ in range(args.warmup):
            for launch in pieces.values():
                launch()
        torch.cuda.synchronize()

        per_round = max(1, args.reps // args.rounds)
        rounds = {name: [] for name in pieces}
        for _r in range(args.rounds):
            ev = {name: [] for name in pieces}
            for _i in range(per_round):
                for name, launch in pieces.items():                 # alternating
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    launch()
                    b.record()
                    ev[name].append((a, b))
            torch.cuda.synchronize()
            for name in pieces:
                rounds[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[name]])))

        def stat(v):
            v = np.array(v)
            return {"median_us": float(np.median(v)), "round_medians_us": [round(float(x), 2) for x in v], "spread_us": float(v.max() - v.min())}

        covered = {n: float(np.mean(c)) for n, c in (("qp_y", want["qp_y"] != 0), ("qp_c", want["qp_c0"] != 0))}
        out = {
            "picture": f"{width}x{height}", "what": label, "units": int(n_units), "ctus": int(n_ctb), "records": {"cu": len(cu), "tu": len(tu)},
            "tables_equal_the_painter": not differing, "differing_tables": differing, "nonzero_fraction": covered,
            "upload_bytes": {"a_three_planes": int(3 * n_units), "b_two_sidecars": int(len(cu) + 2 * len(tu)),
                             "note": "computed from the picture's size and record counts; (a) at pitch = width / 4"},
            "repetitions_per_piece": per_round * args.rounds, "rounds": args.rounds,
            "h2d": {"a_planes_h2d": stat(rounds["a_planes_h2d"]), "b_sidecars_h2d_and_kernel": stat(rounds["b_sidecars_h2d_and_kernel"])},
            "kernel": {"qp_rec_kernel": stat(rounds["qp_rec_kernel"]), "bs_rec_kernel": stat(rounds["bs_rec_kernel"])},
        }
        k = out["kernel"]
        out["kernel"]["qp_rec_not_slower_than_bs_rec"] = bool(k["qp_rec_kernel"]["median_us"] <= k["bs_rec_kernel"]["median_us"])
        return out, differing

    clocks = [clock_state()]
    results, failed = [], []
    for label, w, h, recs in (("bs_rec_cases.BIG", big.width, big.height, list(big.records())),
                              ("BIG tiled 5 x 5 at 1536 x 896, cropped to the picture", 7680, 4320, tiled(big, big.records(), 7680, 4320))):
        r, differing = measure(label, w, h, recs)
        results.append(r)
        failed += differing
    clocks.append(clock_state())
    out = {"tool": "tools/deblock_qp_rec_time.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median of the rounds",
           "clock_state": {"before": clocks[0], "after": clocks[1]},
           "pictures": results}
    print(json.dumps(out, indent=1))
    if failed:
        sys.exit(f"deblock_qp_rec_time: the device's tables differ from the painter's: {failed}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

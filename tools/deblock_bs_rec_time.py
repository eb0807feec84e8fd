"""Times the boundary-strength stage of the bench's 8K picture two ways, in one process, alternating:
  (a) the table path: vvc355_tab_fill_pass with all three record kinds and every side table, then vvc355_deblock_bs_pass;
  (b) the record path: vvc355_tab_fill_pass with the motion records only (the MvField table), then vvc355_deblock_bs_rec_pass.
The picture is bench.py's: BsTables(default_rng(0x5EED0B5), 1920, 4320, 7, split=(0.95, 0.45), cbf_p=0.4) tiled four times across, records
shifted and grouped per CTU like the bench does, all-zero slice and tile maps.  Every piece sits between device events of its own.  The two
paths must leave identical output tables before anything is timed.  A tool, not a test: it needs an MI355X and fails without one; it
reads nothing outside the repository.

    python tools/deblock_bs_rec_time.py [--reps 100] [--rounds 5] [--out profiles/deblock_bs_rec_pass.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every path (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deblock_bs_rec_pass.json"))
    args = ap.parse_args()

    import torch
    import bs_cases
    import bs_rec_cases as rc
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("deblock_bs_rec_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)

    reps = 4
    assert args.width % (reps * 128) == 0
    t = bs_cases.BsTables(np.random.default_rng(0x5EED0B5), args.width // reps, args.height, 7, split=(0.95, 0.45), cbf_p=0.4)
    recs = []
    for r in t.records():
        tiled = np.tile(r, reps)
        tiled["x0"] += (np.arange(len(tiled)) // len(r) * (args.width // reps)).astype(np.int16)
        recs.append(tiled)
    t.width, t.tw, t.cw = args.width, t.tw * reps, t.cw * reps
    n_ctb, n_units = t.cw * t.ch, t.tw * t.th
    groups = [t.group_per_ctu(r, 7, t.cw, n_ctb) for r in recs]
    d_rec = [batch.DeviceBuffer.from_host(g[0].view(np.uint8)) for g in groups]
    d_first = [batch.DeviceBuffer.from_host(g[1]) for g in groups]
    n_rec = tuple(len(g[0]) for g in groups)

    # the tables of both paths: the inputs that travel as they are, the side tables of (a), one MvField table and one set of outputs per path
    small = {"ref_poc": t.ref_poc, "slice_idx": np.zeros(n_ctb, np.int16), "col_bd": np.zeros(t.cw + 1, np.int16), "row_bd": np.zeros(t.ch + 1, np.int16)}
    d_small = {k: batch.DeviceBuffer.from_host(v) for k, v in small.items()}
    itemsize = {name: getattr(t, name).dtype.itemsize for name in t.FILLED}
    side = {name: batch.DeviceBuffer(n_units * itemsize[name]) for name in t.FILLED}
    outs = {p: {name: batch.DeviceBuffer.from_host(np.full(n_units, 0xEE, np.uint8)) for name in t.OUT + rc.TB_C} for p in "ab"}
    mvf_b = batch.DeviceBuffer(n_units * 24)

    def ptr_a(name):
        return d_small[name].ptr if name in d_small else side[name].ptr if name in side else outs["a"][name].ptr

    def ptr_b(name):
        return d_small[name].ptr if name in d_small else mvf_b.ptr if name == "mvf" else outs["b"][name].ptr

    def on_device(f):
        return batch.DeviceBuffer.from_host(np.frombuffer(bytes(f), np.uint8))

    fill_a = t.fill_frame(d_rec[0].ptr, d_rec[1].ptr, d_rec[2].ptr, n_rec, ptr_a, tuple(d.ptr for d in d_first))
    bs_a = t.frame(ptr_a)
    fill_b = t.fill_frame(0, 0, d_rec[2].ptr, (0, 0, n_rec[2]), lambda name: mvf_b.ptr if name == "mvf" else 0, (0, 0, d_first[2].ptr))
    bs_b = rc.rec_frame(t, (d_rec[0].ptr, n_rec[0], d_first[0].ptr), (d_rec[1].ptr, n_rec[1], d_first[1].ptr), ptr_b)
    d_fill_a, d_bs_a, d_fill_b, d_bs_b = on_device(fill_a), on_device(bs_a), on_device(fill_b), on_device(bs_b)
    st = torch.cuda.current_stream().cuda_stream

    def rec_pass(s):
        assert dev.vvc355_deblock_bs_rec_pass(s, d_bs_b.ptr, ctypes.addressof(bs_b)) == 0

    pieces = {
        "a_table_path": [("tab_fill_all", lambda s: dev.vvc355_tab_fill_pass(s, d_fill_a.ptr, ctypes.addressof(fill_a))),
                         ("deblock_bs_pass", lambda s: dev.vvc355_deblock_bs_pass(s, d_bs_a.ptr, ctypes.addressof(bs_a)))],
        "b_record_path": [("tab_fill_motion_only", lambda s: dev.vvc355_tab_fill_pass(s, d_fill_b.ptr, ctypes.addressof(fill_b))),
                          ("deblock_bs_rec_pass", rec_pass)],
    }

    # identical output tables first (this also warms every launch once); (a) leaves tb_*_c among its side tables
    for path in pieces.values():
        for _, launch in path:
            launch(st)
    torch.cuda.synchronize()
    res_a = {name: (side if name in rc.TB_C else outs["a"])[name].to_host(np.uint8, (n_units,)) for name in t.OUT + rc.TB_C}
    res_b = {name: outs["b"][name].to_host(np.uint8, (n_units,)) for name in t.OUT + rc.TB_C}
    differing = [name for name in res_a if not np.array_equal(res_a[name], res_b[name])]
    strengths = sorted(int(v) for v in np.unique(res_a["bs10"]))
    for _ in range(args.warmup):
        for path in pieces.values():
            for _, launch in path:
                launch(st)
    torch.cuda.synchronize()

    per_round = max(1, args.reps // args.rounds)
    rounds = {p: {name: [] for name, _ in path} for p, path in pieces.items()}
    totals = {p: [] for p in pieces}
    for _r in range(args.rounds):
        ev = {p: [] for p in pieces}
        for _i in range(per_round):
            for p, path in pieces.items():                 # alternating: a, b, a, b, ...
                marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(path) + 1)]
                marks[0].record()
                for k, (_, launch) in enumerate(path):
                    launch(st)
                    marks[k + 1].record()
                ev[p].append(marks)
        torch.cuda.synchronize()
        for p, path in pieces.items():
            for k, (name, _) in enumerate(path):
                rounds[p][name].append(float(np.median([m[k].elapsed_time(m[k + 1]) * 1e3 for m in ev[p]])))
            totals[p].append(float(np.median([m[0].elapsed_time(m[-1]) * 1e3 for m in ev[p]])))

    def stat(v):
        v = np.array(v)
        return {"median_us": float(np.median(v)), "round_medians_us": [round(float(x), 2) for x in v], "spread_us": float(v.max() - v.min())}

    # computed, not measured: the intermediate tables a picture in flight holds between the record upload and the deblocking passes
    side_bytes = sum(n_units * itemsize[name] for name in t.FILLED if name != "mvf")
    out = {
        "tool": "tools/deblock_bs_rec_time.py", "picture": f"{args.width}x{args.height}", "device": torch.cuda.get_device_name(0),
        "units": int(n_units), "ctus": int(n_ctb), "records": {"cu": n_rec[0], "tu": n_rec[1], "mv": n_rec[2]},
        "record_bytes": {"cu_tu": int(8 * (n_rec[0] + n_rec[1])), "mv": int(32 * n_rec[2])},
        "repetitions_per_path": per_round * args.rounds, "rounds": args.rounds,
        "identical_outputs": not differing, "differing_tables": differing, "luma_vertical_strengths": strengths,
        "scratch_bytes_per_picture": {"a_table_path": int(side_bytes), "b_record_path": 0,
                                      "note": "side tables other than the MvField table and the outputs (tb_*_c is an output of (b), a side table of (a))"},
        "paths": {},
    }
    for p, path in pieces.items():
        out["paths"][p] = {"total": stat(totals[p]), "pieces": {name: stat(rounds[p][name]) for name, _ in path}}
    a, b = out["paths"]["a_table_path"]["total"], out["paths"]["b_record_path"]["total"]
    spread = max(a["spread_us"], b["spread_us"])
    out["condition"] = {"statement": "median(b) <= median(a) + the run's own spread (the larger of the two paths' max - min over the rounds)",
                        "spread_us": spread, "holds": bool(b["median_us"] <= a["median_us"] + spread)}
    print(json.dumps(out, indent=1))
    if differing:
        sys.exit(f"deblock_bs_rec_time: the two paths do NOT leave identical tables: {differing}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

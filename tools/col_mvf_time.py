"""What vvc355_col_mvf_pass costs on one 7680x4320 picture, next to what it replaces, in the same run (not a pass criterion of any test):

  pass        the hand-back from a full table (n_jobs = 0) and from the unrefined table with the overlay of the DMVR jobs (as many 16x16
              sub-blocks as bench.py's 8K picture has regular inter blocks, drawn with its fractions), COMPRESS on: device events.
  replaced    vvc355_copy_async of the full 49 766 400-byte table (mvf -> dmvr_mvf, the second copy a host had to keep for set_dmvr_info) and
              vvc355_download_async of that table into pinned memory, against vvc355_download_async of the 8 294 400 bytes of entries.
  end to end  pass + download of the entries + synchronisation against copy + download of the table + synchronisation, by wall clock.

The byte counts are exact and asserted.  Both results are compared with the numpy expectation of tests/col_mvf_cases.py before anything is
timed.  Device events around each piece, the pieces alternating inside every repetition, median per round, median and spread (max - min) of
the rounds' medians.  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/col_mvf_time.py [--reps 30] [--rounds 5] [--out profiles/col_mvf.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TABLE_BYTES, ENTRY_BYTES = 49766400, 8294400          # 1920 x 1080 MvField of 24 bytes; 960 x 540 entries of 16


def wall(fn, n=7):
    """Median wall-clock seconds of n calls."""
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def picture(width, height, seed):
    """The MvField table of a picture of bi-predicted 16x16 units, the luma jobs and records of those among them that bench.py's picture
    would predict as regular inter blocks with DMVR, and tab_dmvr_mvf: the table with the records' motion in those blocks."""
    import bench
    import affine_gpm_cases as agc
    import inter_frame_cases as ifc
    rng = np.random.default_rng(seed)
    bw, bh = width // 16, height // 16
    mvf = np.zeros((height // 4, width // 4), ifc.MVF_DT)
    mv = rng.integers(-24 * 16, 24 * 16 + 1, size=(bh, bw, 2, 2))
    mvf["mv"] = mv.repeat(4, axis=0).repeat(4, axis=1)
    mvf["pred_flag"], mvf["ref_idx"] = 3, rng.integers(0, 2, size=(bh, bw, 2)).repeat(4, axis=0).repeat(4, axis=1)
    keep = bench.INTER_FRAC * (1 - bench.CIIP_FRAC / bench.INTER_FRAC) * (1 - bench.AFFINE_FRAC) * (1 - bench.GPM_FRAC)
    by, bx = np.nonzero(rng.random((bh, bw)) < keep)
    jobs = np.zeros(len(bx), agc.BIPRED_JOB_DT)
    jobs["x"], jobs["y"], jobs["w"], jobs["h"], jobs["dmvr"], jobs["pred_flag"] = 16 * bx, 16 * by, 16, 16, 1, 3
    recs = np.zeros((len(bx), 8), np.int32)
    d = rng.integers(-40, 41, size=(len(bx), 2))                          # the refinement: list 0 by +d, list 1 by -d
    recs[:, 0:2], recs[:, 2:4] = mv[by, bx, 0] + d, mv[by, bx, 1] - d
    dmvr = mvf.copy()
    for dy in range(4):
        for dx in range(4):
            e = dmvr[4 * by + dy, 4 * bx + dx]
            e["mv"] = recs[:, :4].reshape(-1, 2, 2)
            dmvr[4 * by + dy, 4 * bx + dx] = e
    return mvf, jobs, recs, dmvr, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of every piece in every round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds; the spread is taken over the rounds' medians")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "col_mvf.json"))
    args = ap.parse_args()

    import torch
    import col_mvf_cases as cm
    from picture_pass_time import clock_state, timed
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("col_mvf_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    clocks = [clock_state()]

    w, h = 7680, 4320
    gw, gh = cm.grid(w, h)
    mvf, jobs, recs, dmvr, keep = picture(w, h, cm.SEED + 900)
    assert mvf.nbytes == dmvr.nbytes == TABLE_BYTES and gw * gh * cm.ENTRY == ENTRY_BYTES and TABLE_BYTES == 6 * ENTRY_BYTES
    d_mvf, d_dmvr, d_jobs, d_recs = cm.up(mvf), cm.up(dmvr), cm.up(jobs), cm.up(recs)
    d_copy = batch.DeviceBuffer(TABLE_BYTES)

    # ---------------------------------------------------------------- both ways, checked before they are timed
    C = abi.COL_MVF_COMPRESS
    runs = {"full_table": cm.ColRun(dev, w, h, d_dmvr.ptr, flags=C),
            "overlay": cm.ColRun(dev, w, h, d_mvf.ptr, flags=C, jobs=d_jobs.ptr, records=d_recs.ptr, n_jobs=len(jobs))}
    want = cm.pack(dmvr, True)
    assert not np.array_equal(want, cm.pack(mvf, True))
    for name, run in runs.items():
        assert run.image.nbytes == ENTRY_BYTES + 2 * cm.SLACK
        bad = run.run(want, st)
        if bad:
            sys.exit(f"col_mvf_time: {name} differs from the numpy expectation ({bad}); nothing timed")
    if not np.array_equal(d_mvf.to_host(np.uint8, (TABLE_BYTES,)), mvf.view(np.uint8).reshape(-1)):
        sys.exit("col_mvf_time: the pass wrote to the table; nothing timed")

    # ---------------------------------------------------------------- what it replaces
    pinned_table, pinned_col = dev.vvc355_host_alloc(TABLE_BYTES), dev.vvc355_host_alloc(ENTRY_BYTES)
    col_ptr = runs["overlay"].frame.col
    pieces = {
        "col_mvf_pass_full_table": lambda: runs["full_table"].issue(st),
        "col_mvf_pass_overlay": lambda: runs["overlay"].issue(st),
        "copy_async_table": lambda: dev.vvc355_copy_async(st, d_copy.ptr, d_mvf.ptr, TABLE_BYTES),
        "download_async_table": lambda: dev.vvc355_download_async(st, pinned_table, d_copy.ptr, TABLE_BYTES),
        "download_async_entries": lambda: dev.vvc355_download_async(st, pinned_col, col_ptr, ENTRY_BYTES),
    }
    t = timed(torch, pieces, args.reps, args.rounds, args.warmup)
    clocks.append(clock_state())
    if dev.vvc355_last_error() != 0:
        sys.exit("col_mvf_time: a HIP error was recorded during the timed loops")
    us = {n: v["gpu"]["median_us"] for n, v in t.items()}

    def after():
        runs["overlay"].issue(st)
        dev.vvc355_download_async(st, pinned_col, col_ptr, ENTRY_BYTES)
        dev.vvc355_stream_sync(st)

    def before():
        dev.vvc355_copy_async(st, d_copy.ptr, d_mvf.ptr, TABLE_BYTES)
        dev.vvc355_download_async(st, pinned_table, d_copy.ptr, TABLE_BYTES)
        dev.vvc355_stream_sync(st)

    t_after, t_before = wall(after), wall(before)
    import ctypes
    got = np.frombuffer(ctypes.string_at(pinned_col, ENTRY_BYTES), "<u4").reshape(gh, gw, 2, 2)
    same = bool(np.array_equal(got, want))
    dev.vvc355_host_free(pinned_table)
    dev.vvc355_host_free(pinned_col)
    if not same:
        sys.exit("col_mvf_time: the pinned copy of the entries differs from the numpy expectation")

    # bytes the pass needs: the entries it reads and the entries it writes; bytes it makes the memory move: the 128-byte lines of the even
    # table rows (every line of them holds an even position), and the entries
    needed = gw * gh * 24 + ENTRY_BYTES
    moved = (h // 8) * (w // 4) * 24 + ENTRY_BYTES
    gbs = lambda nbytes, micro: round(nbytes / micro / 1e3, 1)          # noqa: E731
    out_json = {
        "tool": "tools/col_mvf_time.py", "device": torch.cuda.get_device_name(0),
        "picture": f"{w}x{h}: {h // 4} x {w // 4} MvField, {gh} x {gw} entries; bi-predicted 16x16 units, {len(jobs)} of {(w // 16) * (h // 16)} with DMVR "
                   f"(bench.py's share of regular inter blocks, {keep:.4f})",
        "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median and spread (max - min) of the rounds' medians; end to end: median wall clock",
        "repetitions_per_round": args.reps, "rounds": args.rounds, "result_equals_numpy": True,
        "bytes": {"table": TABLE_BYTES, "entries": ENTRY_BYTES, "table_over_entries": TABLE_BYTES // ENTRY_BYTES, "dmvr_jobs": int(len(jobs)),
                  "pass_needs_read_plus_write": int(needed), "pass_moves_lines_read_plus_write": int(moved), "copy_moves_read_plus_write": 2 * TABLE_BYTES},
        "time": t,
        "rate_GBps": {"pass_full_table_needed_bytes": gbs(needed, us["col_mvf_pass_full_table"]), "pass_full_table_moved_bytes": gbs(moved, us["col_mvf_pass_full_table"]),
                      "copy_async_table": gbs(2 * TABLE_BYTES, us["copy_async_table"]), "download_async_table": gbs(TABLE_BYTES, us["download_async_table"]),
                      "download_async_entries": gbs(ENTRY_BYTES, us["download_async_entries"])},
        "against_what_it_replaces": {
            "pass_over_copy": round(us["col_mvf_pass_full_table"] / us["copy_async_table"], 3),
            "pass_with_overlay_over_copy": round(us["col_mvf_pass_overlay"] / us["copy_async_table"], 3),
            "overlay_launch_us": round(us["col_mvf_pass_overlay"] - us["col_mvf_pass_full_table"], 2),
            "device_leg_before_us": round(us["copy_async_table"] + us["download_async_table"], 1),
            "device_leg_after_us": round(us["col_mvf_pass_overlay"] + us["download_async_entries"], 1),
            "end_to_end_before_s": t_before, "end_to_end_after_s": t_after, "before_over_after": round(t_before / t_after, 2)},
        "clock_state": {"before": clocks[0], "after": clocks[1]},
    }
    print(json.dumps(out_json, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out_json, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

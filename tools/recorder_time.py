"""What the recorder (include/vvc_mi355_rec.h) costs a parser on one 7680x4320 picture (not a pass criterion of any test).  CPU only.

  picture     drawn by tests/ref_recon_cases.draw with bench.py's unit mix: CTU 128, 4:2:0, 10 bit, LMCS with chroma residual scaling,
              dep-quant, bench.INTER_FRAC of the CTUs wholly inter (units up to 128x128), the others intra; about 300 k coded transform blocks.
  recorder    wall time of the picture's vvc355_rec_ctu calls (packing on) plus vvc355_rec_end_picture, and of vvc355_recon_order on the
              CTU table the recorder made (the stand-alone program has a stand-in for it; its time is added to end_picture's).
  pack alone  the same coded blocks through vvc355_levels_pack alone: the part of the work a parser that hands over packed levels cannot avoid.
Timed inside tools/recorder_check.c (--time), built here with the library's flags (-O2) from recorder.c and levels_pack.c: calling the
recorder through ctypes would time ctypes for the 300 k pack calls.  Median and spread (max - min) over the repetitions; the first
repetition, in which the recorder's buffers grow, is reported apart.  There is no threshold; the ratio to pack alone is what to look at.

    python tools/recorder_time.py [--reps 9] [--out profiles/recorder.json]
"""
import argparse
import ctypes
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recorder.json"))
    args = ap.parse_args()

    import bench
    import recorder_cases as rk
    import ref_recon_cases as rc
    from ffvvc_amd import abi

    t0 = time.perf_counter()
    pic = rc.draw("8k", 0x8EC0DE8, bd=10, idc=1, ctb_log2=7, size=(args.width, args.height), intra=1.0, inter_ctu=bench.INTER_FRAC,
                  slices=[(1, 1)], lmcs=bench.LMCS, big_inter=True, min_cu=8)
    first, cus, tus, tbs, levels = rc.shim_arrays(pic)
    n_coded = int((tbs["has_coeffs"] != 0).sum())
    print(f"drawn in {time.perf_counter() - t0:.1f} s: {len(pic.ctus)} CTUs, {len(cus)} units, {n_coded} coded transform blocks", flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "recorder_check"), os.path.join(tmp, "8k.dump")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "recorder_check.c"),
                               os.path.join(ROOT, "ffvvc_amd", "host", "recorder.c"), os.path.join(ROOT, "ffvvc_amd", "host", "levels_pack.c"), "-o", exe])
        rk.dump(pic, dump)
        out = subprocess.check_output([exe, "--time", str(args.reps + 1), dump], text=True)
    rows = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    assert len(rows) == args.reps + 1 and int(rows[0, 3]) == n_coded

    # the ticket order, through the library, on the recorder's own CTU table
    lib = abi.load()
    o = rk.record(lib, pic, True)
    order = np.zeros(len(pic.ctus), np.int32)
    t_order = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        lib.vvc355_recon_order(o.ctus.ctypes.data, pic.ncx, pic.ncy, order.ctypes.data)
        t_order.append(time.perf_counter() - t0)

    def stat(v):
        return dict(median_ms=round(1e3 * float(np.median(v)), 3), spread_ms=round(1e3 * float(np.max(v) - np.min(v)), 3))

    warm = rows[1:]
    rec_total = warm[:, 0] + warm[:, 1] + float(np.median(t_order))
    result = {
        "tool": "tools/recorder_time.py", "cpu": cpu_model(), "threads": 1, "reps": args.reps,
        "picture": dict(width=args.width, height=args.height, ctb=128, chroma_format_idc=1, bit_depth=10, lmcs=bool(bench.LMCS),
                        inter_ctu_frac=bench.INTER_FRAC, ctus=len(pic.ctus), units=len(cus), transform_units=int(len(tus)),
                        coded_transform_blocks=n_coded, commands=int(rows[0, 4]), records=int(rows[0, 5]), level_bytes_int32=int(4 * len(levels))),
        "recorder": dict(rec_ctu_calls=stat(warm[:, 0]), end_picture=stat(warm[:, 1]), recon_order=stat(t_order), total=stat(rec_total),
                         first_picture_ms=round(1e3 * float(rows[0, 0] + rows[0, 1]), 3), late_keep=int(o.late_keep),
                         stats=o.stats),
        "levels_pack_alone": stat(warm[:, 2]),
        "ratio_total_to_pack_alone": round(float(np.median(rec_total) / np.median(warm[:, 2])), 2),
        "per_block_ns": dict(recorder=round(1e9 * float(np.median(rec_total)) / n_coded, 1), pack_alone=round(1e9 * float(np.median(warm[:, 2])) / n_coded, 1)),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

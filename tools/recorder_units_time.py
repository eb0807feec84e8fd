"""What the unit entry of the recorder (vvc355_rec_ctu_units, include/vvc_mi355_rec.h) costs a parser on one 7680x4320 picture next to
vvc355_rec_ctu, which this work leaves as it was (not a pass criterion of any test).  CPU only, one core.

  picture     tools/recorder_time.py's: tests/ref_recon_cases.draw with bench.py's unit mix (CTU 128, 4:2:0, 10 bit, LMCS with chroma residual
              scaling, dep-quant, bench.INTER_FRAC of the CTUs wholly inter), dressed by tests/recorder_units_cases.dress with NO CIIP unit, so
              that both entries accept it: a prediction unit for every inter unit (PLAIN, sub-block PLAIN, AFFINE, GPM), transform units for
              the uncoded units.
  both ways   wall time of the picture's CTU calls (packing on) plus vvc355_rec_end_picture through vvc355_rec_ctu and through
              vvc355_rec_ctu_units, alternating inside one process and one recorder object.
Timed inside tools/recorder_units_check.c (--time), built here with the library's flags (-O2) from recorder.c and levels_pack.c, pinned to
one core (--cpu).  Median and spread (max - min) over the repetitions; the first repetition, in which the recorder's buffers grow, is left
out.  The two entries alternate inside every repetition, so the cost of the extra lists is taken PAIRED: the difference of the two totals
per repetition, its median and its quartiles, which a slow stretch of the machine moves far less than it moves either total.  No threshold:
the ratio and the extra time per coding unit, with the quartiles, are what to look at.

    python tools/recorder_units_time.py [--reps 25] [--cpu 0] [--out profiles/recorder_units.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--cpu", type=int, default=0)
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recorder_units.json"))
    args = ap.parse_args()

    import bench
    import recorder_units_cases as uc
    import ref_recon_cases as rc
    from recorder_time import cpu_model

    t0 = time.perf_counter()
    pic = uc.dress(rc.draw("8k", 0x8EC0DE8, bd=10, idc=1, ctb_log2=7, size=(args.width, args.height), intra=1.0, inter_ctu=bench.INTER_FRAC,
                           slices=[(1, 1)], lmcs=bench.LMCS, big_inter=True, min_cu=8), 8000, 0.0)
    units = [cu for ctu in pic.ctus for cu in ctu]
    kinds = np.bincount([cu["pu"]["kind"] for cu in units if "pu" in cu], minlength=3)
    n_mvf = sum(cu["pu"]["nsx"] * cu["pu"]["nsy"] if "pu" in cu else 1 for cu in units)
    n_tu = sum(len(cu["tus"]) * 2 for cu in units)
    print(f"drawn in {time.perf_counter() - t0:.1f} s: {len(pic.ctus)} CTUs, {len(units)} units", flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "recorder_units_check"), os.path.join(tmp, "8k.dump")
        subprocess.check_call(["cc", "-O2", "-std=c11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "recorder_units_check.c"),
                               os.path.join(ROOT, "ffvvc_amd", "host", "recorder.c"), os.path.join(ROOT, "ffvvc_amd", "host", "levels_pack.c"), "-o", exe])
        uc.dump(pic, dump)
        out = subprocess.check_output(["taskset", "-c", str(args.cpu), exe, "--time", str(args.reps + 1), dump] if os.path.exists("/usr/bin/taskset") else
                                      [exe, "--time", str(args.reps + 1), dump], text=True)
    rows = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    assert len(rows) == args.reps + 1 and int(rows[0, 4]) == len(units)

    def stat(v):
        return dict(median_ms=round(1e3 * float(np.median(v)), 3), spread_ms=round(1e3 * float(np.max(v) - np.min(v)), 3))

    warm = rows[1:]
    walk, both = warm[:, 0] + warm[:, 1], warm[:, 2] + warm[:, 3]
    paired = both - walk
    q1, extra, q3 = (float(v) for v in np.percentile(paired, [25, 50, 75]))
    n_rec = len(units) + n_tu + n_mvf
    result = {
        "tool": "tools/recorder_units_time.py", "cpu": cpu_model(), "threads": 1, "reps": args.reps,
        "picture": dict(width=args.width, height=args.height, ctb=128, chroma_format_idc=1, bit_depth=10, lmcs=bool(bench.LMCS),
                        inter_ctu_frac=bench.INTER_FRAC, ctus=len(pic.ctus), units=len(units), inter_units=int(kinds.sum()),
                        plain=int(kinds[0]), affine=int(kinds[1]), gpm=int(kinds[2]), ciip=0, cu_records=len(units), tu_records=n_tu, mvf_unit_records=n_mvf),
        "rec_ctu": dict(ctu_calls=stat(warm[:, 0]), end_picture=stat(warm[:, 1]), total=stat(walk)),
        "rec_ctu_units": dict(ctu_calls=stat(warm[:, 2]), end_picture=stat(warm[:, 3]), total=stat(both)),
        "ratio_units_to_rec_ctu": round(float(np.median(both / walk)), 3),
        "ratio_quartiles": [round(float(v), 3) for v in np.percentile(both / walk, [25, 75])],
        "paired_extra_ms": dict(median=round(1e3 * extra, 3), q1=round(1e3 * q1, 3), q3=round(1e3 * q3, 3)),
        "extra_ns_per_unit": dict(median=round(1e9 * extra / len(units), 1), q1=round(1e9 * q1 / len(units), 1), q3=round(1e9 * q3 / len(units), 1)),
        "extra_ns_per_record": dict(median=round(1e9 * extra / n_rec, 1), q1=round(1e9 * q1 / n_rec, 1), q3=round(1e9 * q3 / n_rec, 1)),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()

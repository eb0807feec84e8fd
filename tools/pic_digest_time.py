"""What vvc355_pic_digest_pass costs on one 7680x4320 10-bit 4:2:0 picture (99.5 MB in HBM), against what a host had to do for the same
numbers before it existed, in the same run (not a pass criterion of any test):

  digest      the pass with what = 1 (Adler-32), 2 (checksum), 4 (CRC) and 7 (all): device events around the two launches.
  before      vvc355_download of the three planes (wall clock, the link) plus zlib.adler32, binascii.crc_hqx and the numpy checksum of
              tests/pic_digest_cases.py on the host (wall clock).
  streaming   vvc355_lmcs_frame_pass on the luma plane, every slice mapped: this library's own figure for a pass that streams a plane
              (it reads and writes the plane; the digest only reads).

The 8K result is compared with the stdlib values before anything is timed.  Device events around each piece, the pieces alternating inside
every repetition, median per round, median and spread (max - min) of the rounds' medians.  A tool, not a test: it needs an MI355X and fails
without one; it reads nothing outside the repository.

    python tools/pic_digest_time.py [--reps 30] [--rounds 5] [--out profiles/pic_digest.json]
"""
import argparse
import binascii
import ctypes
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def wall(fn, n=5):
    """Median wall-clock seconds of n calls."""
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions of every piece in every round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds; the spread is taken over the rounds' medians")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pic_digest.json"))
    args = ap.parse_args()

    import torch
    import pic_digest_cases as dc
    import picture_cases as pcs
    from picture_pass_time import clock_state, timed
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("pic_digest_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    clocks = [clock_state()]

    bd, w, h = 10, 7680, 4320
    rng = np.random.default_rng(dc.SEED + 900)
    planes = [rng.integers(0, 1 << bd, size=(ph, pw), dtype=np.uint16) for (pw, ph) in dc.chroma_dims(w, h, 420)]
    pic = dc.DevicePicture(bd, planes)
    n_bytes = sum(p.nbytes for p in planes)

    # ---------------------------------------------------------------- before: the download and the host digests
    host_copies = [np.empty_like(img) for img in pic.images]

    def download():
        for b, out in zip(pic.bufs, host_copies):
            dev.vvc355_download(out.ctypes.data, b.ptr, out.nbytes)

    t_download = wall(download)
    data = [dc.plane_bytes(p, bd) for p in planes]
    t_adler = wall(lambda: [zlib.adler32(b"".join(data), 0)] + [zlib.adler32(d, 0) for d in data], 3)
    t_crc = wall(lambda: [binascii.crc_hqx(d, dc.CRC_INIT) for d in data], 3)
    t_sum = wall(lambda: [dc.checksum_numpy(p, bd) for p in planes], 3)
    want = dc.expected(planes, bd)

    # ---------------------------------------------------------------- the pass, checked before it is timed
    runs = {what: dc.Run.on(pic, what) for what in (1, 2, 4, 7)}
    for what, run in runs.items():
        assert run.issue(st) == 0
        torch.cuda.synchronize()
        got, intact = run.result()
        if got != dc.expected(planes, bd, what) or not intact or dev.vvc355_last_error() != 0:
            sys.exit(f"pic_digest_time: what = {what} differs from the stdlib values ({dc.describe(got, dc.expected(planes, bd, what))}); nothing timed")

    # ---------------------------------------------------------------- streaming: inverse LMCS of the luma plane
    k = pcs.Keep()
    cw, ch = (w + 127) >> 7, (h + 127) >> 7
    c = pcs.SimpleNamespace(bd=bd, width=w, height=h, ctb_log2=7, cw=cw, ch=ch, pitch=pic.pitch[0], isz=2, n_slices=1,
                            slice_idx=np.zeros(cw * ch, np.int16), used=np.ones(1, np.uint8), lut=rng.permutation(1 << bd).astype(np.uint16))
    d_luma = k.up(pic.images[0])
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_luma.ptr, k.up(c.lut).ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))

    def lmcs():
        assert dev.vvc355_lmcs_frame_pass(st, bd, lf_ptr, ctypes.addressof(lf)) == 0

    pieces = {f"digest_what_{what}": (lambda run=run: run.issue(st)) for what, run in runs.items()}
    pieces["lmcs_frame_pass_luma"] = lmcs
    t = timed(torch, pieces, args.reps, args.rounds, args.warmup)
    clocks.append(clock_state())
    if dev.vvc355_last_error() != 0:
        sys.exit("pic_digest_time: a HIP error was recorded during the timed loops")

    us = {n: v["gpu"]["median_us"] for n, v in t.items()}
    gbs = lambda nbytes, micro: round(nbytes / micro / 1e3, 1)          # noqa: E731
    host_digests = {"adler32_total_and_per_plane_s": t_adler, "crc_hqx_s": t_crc, "numpy_checksum_s": t_sum}
    before_us = {1: (t_download + t_adler) * 1e6, 2: (t_download + t_sum) * 1e6, 4: (t_download + t_crc) * 1e6, 7: (t_download + t_adler + t_crc + t_sum) * 1e6}
    out_json = {
        "tool": "tools/pic_digest_time.py", "device": torch.cuda.get_device_name(0),
        "picture": f"{w}x{h}, {bd} bit, 4:2:0, pitch a multiple of 256 bytes", "picture_bytes": int(n_bytes),
        "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median and spread (max - min) of the rounds' medians; host pieces: median wall clock",
        "repetitions_per_round": args.reps, "rounds": args.rounds,
        "result_equals_stdlib_values": True, "result": want,
        "workgroups_of_the_partials_kernel": int(runs[7].groups), "work_bytes": int(runs[7].work_bytes),
        "time": t,
        "digest_read_rate_GBps": {n: gbs(n_bytes, us[n]) for n in us if n.startswith("digest")},
        "before": {"download_three_planes_s": t_download, "download_GBps": round(sum(x.nbytes for x in host_copies) / t_download / 1e9, 1),
                   "host_digests": host_digests},
        "comparison_with_before": {
            f"what_{what}": {"pass_us": us[f"digest_what_{what}"], "download_alone_us": t_download * 1e6, "download_plus_host_digests_us": before_us[what],
                             "pass_beats_the_download_alone": bool(us[f"digest_what_{what}"] < t_download * 1e6),
                             "download_alone_over_pass": round(t_download * 1e6 / us[f"digest_what_{what}"], 1),
                             "before_over_pass": round(before_us[what] / us[f"digest_what_{what}"], 1)} for what in (1, 2, 4, 7)},
        "comparison_with_lmcs_frame_pass": {
            "lmcs_us": us["lmcs_frame_pass_luma"], "lmcs_bytes_read": int(planes[0].nbytes), "lmcs_bytes_written": int(planes[0].nbytes),
            "lmcs_read_rate_GBps": gbs(planes[0].nbytes, us["lmcs_frame_pass_luma"]),
            "lmcs_read_plus_write_rate_GBps": gbs(2 * planes[0].nbytes, us["lmcs_frame_pass_luma"]),
            "digest_what_1_read_rate_GBps": gbs(n_bytes, us["digest_what_1"])},
        "clock_state": {"before": clocks[0], "after": clocks[1]},
    }
    print(json.dumps(out_json, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out_json, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

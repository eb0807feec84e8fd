"""What vvc355_pic_output_pass costs on one 7680x4320 10-bit 4:2:0 picture (99.5 MB in HBM), against the device's own figure for the same
traffic, the library's other streaming passes, and what a host had to do before it existed, in the same run (not a pass criterion of any test):

  output      the pass as planar as stored into compact planes (yuv420p10le), as P010 and as 8-bit NV12: device events around the launch.
  copy        (a) vvc355_copy_async, device to device, of as many bytes as the as-stored mode reads and writes.
  streaming   (b) vvc355_pic_digest_pass (Adler-32, reads the picture) and vvc355_lmcs_frame_pass on the luma plane (reads and writes it).
  before      (c) vvc355_download of the three pitched planes plus the numpy repack of tests/pic_output_cases.py, against the pass plus
              vvc355_download_async of the packed bytes into pinned memory, both by wall clock up to the stream's synchronisation.

Every mode's result is compared with numpy before anything is timed.  Device events around each piece, the pieces alternating inside every
repetition, median per round, median and spread (max - min) of the rounds' medians.  A tool, not a test: it needs an MI355X and fails without
one; it reads nothing outside the repository.

    python tools/pic_output_time.py [--reps 30] [--rounds 5] [--out profiles/pic_output.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pic_output.json"))
    args = ap.parse_args()

    import torch
    import pic_digest_cases as dc
    import pic_output_cases as oc
    import picture_cases as pcs
    from picture_pass_time import clock_state, timed
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("pic_output_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    clocks = [clock_state()]

    bd, w, h = 10, 7680, 4320
    rng = np.random.default_rng(oc.SEED + 900)
    planes = [rng.integers(0, 1 << bd, size=(ph, pw), dtype=np.uint16) for (pw, ph) in dc.chroma_dims(w, h, 420)]
    pic = dc.DevicePicture(bd, planes)
    n_bytes = sum(p.nbytes for p in planes)

    # ---------------------------------------------------------------- the three modes, compact destinations, checked before they are timed
    modes = {"planar_as_stored": (abi.OUT_PLANAR, bd, False), "p010": (abi.OUT_SEMI, 16, False), "nv12_8bit": (abi.OUT_SEMI, 8, False)}
    runs, out_bytes = {}, {}
    for name, mode in modes.items():
        run = oc.OutRun.on(pic, mode, pitch="compact")
        assert run.issue(st) == 0
        torch.cuda.synchronize()
        bad = run.mismatch(planes)
        if bad or dev.vvc355_last_error() != 0:
            sys.exit(f"pic_output_time: {name} differs from the numpy expectation ({bad}); nothing timed")
        runs[name], out_bytes[name] = run, int(sum(hh * rb for (_, hh), rb in zip(run.out_dims, run.rowbytes)))
    if any(not np.array_equal(a, b) for a, b in zip(pic.download(), pic.images)):
        sys.exit("pic_output_time: the pass wrote to a source plane; nothing timed")

    # ---------------------------------------------------------------- (a) the device's own copy of the as-stored mode's traffic
    d_a, d_b = batch.DeviceBuffer(n_bytes), batch.DeviceBuffer(n_bytes)

    def copy():
        dev.vvc355_copy_async(st, d_b.ptr, d_a.ptr, n_bytes)

    # ---------------------------------------------------------------- (b) the library's streaming passes
    digest = dc.Run.on(pic, abi.DIGEST_ADLER32)
    k = pcs.Keep()
    cw, ch = (w + 127) >> 7, (h + 127) >> 7
    c = pcs.SimpleNamespace(bd=bd, width=w, height=h, ctb_log2=7, cw=cw, ch=ch, pitch=pic.pitch[0], isz=2, n_slices=1,
                            slice_idx=np.zeros(cw * ch, np.int16), used=np.ones(1, np.uint8), lut=rng.permutation(1 << bd).astype(np.uint16))
    d_luma = k.up(pic.images[0])
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_luma.ptr, k.up(c.lut).ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))

    def lmcs():
        assert dev.vvc355_lmcs_frame_pass(st, bd, lf_ptr, ctypes.addressof(lf)) == 0

    pieces = {f"output_{name}": (lambda run=run: run.issue(st)) for name, run in runs.items()}
    pieces["copy_async_same_bytes"] = copy
    pieces["digest_adler32"] = lambda: digest.issue(st)
    pieces["lmcs_frame_pass_luma"] = lmcs
    t = timed(torch, pieces, args.reps, args.rounds, args.warmup)
    clocks.append(clock_state())
    if dev.vvc355_last_error() != 0:
        sys.exit("pic_output_time: a HIP error was recorded during the timed loops")
    us = {n: v["gpu"]["median_us"] for n, v in t.items()}

    # ---------------------------------------------------------------- (c) what the pass replaces, by wall clock
    host_copies = [np.empty_like(img) for img in pic.images]

    def download():
        for b, out in zip(pic.bufs, host_copies):
            dev.vvc355_download(out.ctypes.data, b.ptr, out.nbytes)

    t_download = wall(download)
    replaced = {}
    for name, mode in modes.items():
        run = runs[name]
        t_repack = wall(lambda: [oc.sample_bytes(o).tobytes() for o in oc.out_planes(planes, bd, *mode)], 3)
        sizes = [hh * rb for (_, hh), rb in zip(run.out_dims, run.rowbytes)]
        pinned = dev.vvc355_host_alloc(sum(sizes))

        def packed(run=run, sizes=sizes, pinned=pinned):
            run.issue(st)
            at = 0
            for p, n in enumerate(sizes):
                dev.vvc355_download_async(st, pinned + at, run.frame.dst[p], n)
                at += n
            dev.vvc355_stream_sync(st)

        t_packed = wall(packed)
        got = np.frombuffer(ctypes.string_at(pinned, sum(sizes)), np.uint8)
        same = bool(np.array_equal(got, np.concatenate([oc.sample_bytes(o).reshape(-1) for o in oc.out_planes(planes, bd, *mode)])))
        dev.vvc355_host_free(pinned)
        if not same:
            sys.exit(f"pic_output_time: {name}: the pinned copy differs from the numpy expectation")
        replaced[name] = {"download_pitched_planes_s": t_download, "numpy_repack_s": t_repack, "before_s": t_download + t_repack,
                          "pass_plus_download_async_s": t_packed, "packed_bytes": int(sum(sizes)), "before_over_after": round((t_download + t_repack) / t_packed, 1),
                          "download_alone_over_after": round(t_download / t_packed, 2)}

    gbs = lambda nbytes, micro: round(nbytes / micro / 1e3, 1)          # noqa: E731
    spread = t["copy_async_same_bytes"]["gpu"]["spread_us"]
    out_json = {
        "tool": "tools/pic_output_time.py", "device": torch.cuda.get_device_name(0),
        "picture": f"{w}x{h}, {bd} bit, 4:2:0, pitch a multiple of 256 bytes", "picture_bytes": int(n_bytes),
        "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median and spread (max - min) of the rounds' medians; (c): median wall clock",
        "repetitions_per_round": args.reps, "rounds": args.rounds, "result_equals_numpy": True,
        "segments": {n: int(r.segments()) for n, r in runs.items()},
        "time": t,
        "bytes": {n: {"read": int(n_bytes), "written": out_bytes[n]} for n in modes},
        "read_plus_write_rate_GBps": dict({f"output_{n}": gbs(n_bytes + out_bytes[n], us[f"output_{n}"]) for n in modes},
                                          copy_async_same_bytes=gbs(2 * n_bytes, us["copy_async_same_bytes"]),
                                          lmcs_frame_pass_luma=gbs(2 * planes[0].nbytes, us["lmcs_frame_pass_luma"])),
        "read_rate_GBps": {"digest_adler32": gbs(n_bytes, us["digest_adler32"])},
        "as_stored_against_the_copy": {
            "pass_us": us["output_planar_as_stored"], "copy_us": us["copy_async_same_bytes"], "copy_spread_us": spread,
            "target_us": us["copy_async_same_bytes"] + spread, "within_target": bool(us["output_planar_as_stored"] <= us["copy_async_same_bytes"] + spread),
            "pass_over_copy": round(us["output_planar_as_stored"] / us["copy_async_same_bytes"], 3)},
        "what_it_replaces": replaced,
        "clock_state": {"before": clocks[0], "after": clocks[1]},
    }
    print(json.dumps(out_json, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out_json, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

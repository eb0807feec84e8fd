"""Two measurements for vvc355_picture_pass and the inverse-LMCS stage driver that came with it (not a pass criterion of any test):

  (a) inverse LMCS   vvc355_lmcs_frame_pass (no job array: a workgroup finds its CTB's slice) against vvc355_lmcs_batch on one host-built
                     vvc355_blend_job per CTB, on an 8K 10-bit luma plane (7680x4320, CTU 128, pitch a multiple of 256 bytes) with every
                     slice using LMCS, in the same run.  The two move the same bytes; both must leave the same plane before anything is timed.
  (b) a picture      the filter half of a picture on the record path — tab_fill (motion), bs_rec, qp_rec, both deblocking directions, SAO,
                     the ALF build and filter — as ONE vvc355_picture_pass against the same stage entries called one by one in the documented
                     order, on the C0 recipe of tests/ref_pass_cases.py drawn at --width x --height (default 1480x840, 10 bit, 4:2:0, CTU 64).
                     GPU time = device events around the calls (first launch to the end of the last stage); host time = wall clock inside
                     the call(s), the stream idle before each.  Both forms must leave the same planes.
                     (The tests' picture of both halves, ciip_frame_cases.e2e_work() with records derived from its units, is a fixed
                     256x192 picture: at that size every stage is launch overhead.  The reconstruction stages in front of the filters
                     are the same launches in either form, so the filter half at a size whose kernels do work stands for the call.)

Device events around each piece, the pieces alternating inside every repetition, median per round, median and spread (max - min) of the
rounds' medians.  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/picture_pass_time.py [--reps 50] [--rounds 5] [--out profiles/picture_pass.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clock_state():
    """The clocks as the driver reports them (read only), before and after the timed loops."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, timeout=60, text=True)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr[-200:]}
    except Exception as e:                    # no tool, no permission: say so in the profile instead of failing the measurement
        return {"unavailable": repr(e)}


def stat(v):
    v = np.array(v)
    return {"median_us": float(np.median(v)), "round_medians_us": [round(float(x), 2) for x in v], "spread_us": float(v.max() - v.min())}


def timed(torch, pieces, reps, rounds, warmup, host=False):
    """{name: stat} of GPU time per piece (and of host time inside the call with host=True: the stream is drained before each call then)."""
    for _ in range(warmup):
        for launch in pieces.values():
            launch()
    torch.cuda.synchronize()
    gpu, cpu = {n: [] for n in pieces}, {n: [] for n in pieces}
    for _r in range(rounds):
        ev, wall = {n: [] for n in pieces}, {n: [] for n in pieces}
        for _i in range(reps):
            for name, launch in pieces.items():                 # alternating
                if host:
                    torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t0 = time.perf_counter()
                launch()
                wall[name].append((time.perf_counter() - t0) * 1e6)
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        for name in pieces:
            gpu[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[name]])))
            cpu[name].append(float(np.median(wall[name])))
    out = {n: {"gpu": stat(gpu[n])} for n in pieces}
    if host:
        for n in pieces:
            out[n]["host_in_call"] = stat(cpu[n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1480, help="(b): luma width of the picture, a multiple of 8")
    ap.add_argument("--height", type=int, default=840)
    ap.add_argument("--reps", type=int, default=50, help="timed repetitions of every piece in every round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds; the spread is taken over the rounds' medians")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picture_pass.json"))
    args = ap.parse_args()

    import torch
    import bs_rec_cases as rc
    import picture_cases as pcs
    import qp_rec_cases as qc
    import ref_pass_cases as pc
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("picture_pass_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    k = pcs.Keep()
    clocks = [clock_state()]

    # ---------------------------------------------------------------- (a) inverse LMCS on an 8K luma plane
    bd, w, h, log2 = 10, 7680, 4320, 7
    rng = np.random.default_rng(pcs.SEED + 900)
    cw, ch = (w + 127) >> 7, (h + 127) >> 7
    c = pcs.SimpleNamespace(bd=bd, width=w, height=h, ctb_log2=log2, cw=cw, ch=ch, pitch=batch.plane_pitch(w, 2), isz=2, n_slices=4,
                            slice_idx=np.minimum(np.arange(cw * ch) * 4 // (cw * ch), 3).astype(np.int16), used=np.ones(4, np.uint8),
                            plane=rng.integers(0, 1 << bd, size=(h, w), dtype=np.int64).astype(np.uint16),
                            lut=rng.permutation(1 << bd).astype(np.uint16))
    image = batch.to_pitched(c.plane)
    d_a, d_b, d_lut = k.up(image), k.up(image), k.up(c.lut)
    lf_ptr, lf = k.frame(pcs.lmcs_frame(c, d_a.ptr, d_lut.ptr, k.up(c.slice_idx).ptr, k.up(c.used).ptr))
    jobs = pcs.lmcs_jobs(c, d_b.ptr, d_lut.ptr)
    d_jobs = k.up(jobs)

    def frame_pass():
        assert dev.vvc355_lmcs_frame_pass(st, bd, lf_ptr, ctypes.addressof(lf)) == 0

    def batch_on_jobs():
        dev.vvc355_lmcs_batch(st, bd, d_jobs.ptr, len(jobs), 128, 128)

    frame_pass()
    batch_on_jobs()
    torch.cuda.synchronize()
    got_a, got_b = d_a.to_host(np.uint16, image.shape), d_b.to_host(np.uint16, image.shape)
    want = image.copy()
    want[:, :w] = c.lut[c.plane]
    lmcs_equal = bool(np.array_equal(got_a, want) and np.array_equal(got_b, want))
    if not lmcs_equal or dev.vvc355_last_error() != 0:
        sys.exit("picture_pass_time: the two inverse-LMCS paths do not both equal the numpy lookup; nothing timed")
    t_lmcs = timed(torch, {"lmcs_frame_pass": frame_pass, "lmcs_batch_on_per_ctb_jobs": batch_on_jobs}, args.reps, args.rounds, args.warmup)
    ga, gb = t_lmcs["lmcs_frame_pass"]["gpu"], t_lmcs["lmcs_batch_on_per_ctb_jobs"]["gpu"]
    lmcs_gap = abs(ga["median_us"] - gb["median_us"])

    # ---------------------------------------------------------------- (b) the filter half of a picture, one call against stage by stage
    rng = np.random.default_rng(pc.SEED + 900)
    dp = pc.draw_deblock("T0", rng, 10, (1, 1), 3, 6, (args.width, args.height), 3, True, (0, 0), True, split=(0.9, 0.5))
    fp = pc.draw_filter("T0", rng, 10, (1, 1), 3, 6, None, 3, True, (0, 0), t=dp.t, planes=False)
    t, p = dp.t, dp.rec
    (cu, cu_first), (tu, tu_first), (mv, mv_first) = rc.grouped(t)
    tabs = {n: k.up(np.full((t.th, t.tw), 0xEE, np.uint8)) for n in t.OUT + rc.TB_C + qc.TABLES}
    tabs["mvf"] = batch.DeviceBuffer(t.mvf.nbytes)
    for n in ("ref_poc", "slice_idx", "col_bd", "row_bd"):
        tabs[n] = k.up(getattr(t, n))
    tabs["dbp"], tabs["sao"], tabs["alf"] = k.up(dp.arrays["dbp"]), k.up(fp.sao), k.up(fp.alf)
    tabs["slices"] = k.up(np.frombuffer(bytes(pc.alf_slices(fp, [k.up(a).ptr for a in fp.aps])), np.uint8))
    addr = lambda n: tabs[n].ptr          # noqa: E731
    d_cu, d_cu_first, d_tu, d_tu_first, d_cu_qp, d_tu_qp_c, d_mv, d_mv_first = (k.up(a) for a in (cu, cu_first, tu, tu_first, p.cu_qp, p.tu_qp_c, mv, mv_first))
    cu_arg, tu_arg = (d_cu.ptr, len(cu), d_cu_first.ptr), (d_tu.ptr, len(tu), d_tu_first.ptr)
    start = [batch.to_pitched(pl) for pl in dp.planes]
    strides = [q.strides[0] for q in start]
    rec, sao, out = ([k.up(q) for q in start] for _ in range(3))
    ptrs = lambda bufs: [b.ptr for b in bufs]          # noqa: E731
    frames = dict(
        tab_fill=t.fill_frame(0, 0, d_mv.ptr, (0, 0, len(mv)), lambda name: tabs["mvf"].ptr if name == "mvf" else 0, (0, 0, d_mv_first.ptr)),
        bs_rec=rc.rec_frame(t, cu_arg, tu_arg, addr, 3, tb_c=True),
        qp_rec=qc.qp_frame(t, cu_arg, tu_arg, d_cu_qp.ptr, d_tu_qp_c.ptr, [tabs[n].ptr for n in qc.TABLES], t.tw, 3),
        deblock_v=pc.deblock_frame(dp, 1, ptrs(rec), strides, addr), deblock_h=pc.deblock_frame(dp, 0, ptrs(rec), strides, addr),
        sao=pc.sao_frame(fp, ptrs(sao), ptrs(rec), strides, strides, addr), alf=pc.alf_frame(fp, ptrs(out), ptrs(sao), strides, strides, addr))
    stages = {n: k.frame(f) for n, f in frames.items()}
    work = k.up(np.zeros(dev.vvc355_alf_frame_work_bytes(t.cw * t.ch), np.uint8)).ptr
    pic = pcs.picture(stages, alf_work=work)
    a_of = {n: (ptr, ctypes.addressof(f)) for n, (ptr, f) in stages.items()}

    def restore():
        for b, q in zip(rec, start):
            dev.vvc355_upload(b.ptr, q.ctypes.data, q.nbytes)

    def one_call():
        assert dev.vvc355_picture_pass(st, 10, ctypes.addressof(pic)) == 0

    def stage_by_stage():
        dev.vvc355_tab_fill_pass(st, *a_of["tab_fill"])
        dev.vvc355_deblock_bs_rec_pass(st, *a_of["bs_rec"])
        dev.vvc355_deblock_qp_rec_pass(st, *a_of["qp_rec"])
        dev.vvc355_alf_frame_build(st, 10, *a_of["alf"], work)
        dev.vvc355_deblock_frame_pass(st, 10, *a_of["deblock_v"])
        dev.vvc355_deblock_frame_pass(st, 10, *a_of["deblock_h"])
        dev.vvc355_sao_frame_pass(st, 10, *a_of["sao"])
        dev.vvc355_alf_frame_filter(st, 10, a_of["alf"][1], work)

    results = []
    for launch in (one_call, stage_by_stage):
        restore()
        launch()
        torch.cuda.synchronize()
        results.append([b.to_host(np.uint8, (b.nbytes,)) for b in rec + sao + out])
    picture_equal = all(np.array_equal(x, y) for x, y in zip(*results)) and any(np.any(x != q.view(np.uint8).ravel()) for x, q in zip(results[0][6:], start))
    if not picture_equal or dev.vvc355_last_error() != 0:
        sys.exit("picture_pass_time: one call and stage by stage leave different planes; nothing timed")
    # (the timed repetitions deblock planes that are already deblocked: the work per launch does not depend on the samples)
    t_pic = timed(torch, {"picture_pass": one_call, "stage_by_stage": stage_by_stage}, args.reps, args.rounds, args.warmup, host=True)
    clocks.append(clock_state())

    out_json = {
        "tool": "tools/picture_pass_time.py", "device": torch.cuda.get_device_name(0),
        "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median and spread (max - min) of the rounds' medians",
        "repetitions_per_round": args.reps, "rounds": args.rounds,
        "a_inverse_lmcs": {
            "picture": "7680x4320 luma, 10 bit, CTU 128, four slices, every slice with sh_lmcs_used_flag", "ctbs": int(cw * ch), "jobs_of_the_batch_path": int(len(jobs)),
            "upload_bytes": {"frame_pass": int(ctypes.sizeof(abi.LmcsFrame) + c.slice_idx.nbytes + c.used.nbytes), "batch_jobs": int(jobs.nbytes)},
            "both_equal_the_numpy_lookup": lmcs_equal, "time": t_lmcs, "gap_us": lmcs_gap,
            "gap_within_run_to_run_spread": bool(lmcs_gap <= max(ga["spread_us"], gb["spread_us"]))},
        "b_picture": {
            "picture": f"{args.width}x{args.height}, 10 bit, 4:2:0, CTU 64, three slices, tiles: the C0 recipe of tests/ref_pass_cases.py",
            "stages": list(frames), "records": {"cu": int(len(cu)), "tu": int(len(tu)), "mv": int(len(mv))},
            "both_forms_leave_identical_planes": bool(picture_equal), "time": t_pic,
            "note": "host_in_call: wall clock inside vvc355_picture_pass / inside the eight stage calls (through ctypes), the stream drained before each"},
        "clock_state": {"before": clocks[0], "after": clocks[1]},
    }
    print(json.dumps(out_json, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out_json, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""What vvc355_ciip_frame_pass costs next to the host-built path it replaces, on the bench picture's CIIP population: the combined inter /
intra coding units of recon_cases.ReconWork with the ciip_ctu mask bench.py draws (same seeds, same CTU kinds; 7680x4320 by default:
whole CTUs of 32x32 CIIP units, bi-predicted, motion within +-24 samples, LMCS on).  Two groups of numbers:
  bytes    what a caller uploads per picture: one 32-byte vvc355_ciip_cu per unit against the host-built vvc355_bipred_job array (104 bytes
           per tile).  Computed from the counts, not measured.  (The command array is uploaded either way.)
  time     (a) vvc355_ciip_frame_pass = builder kernel (jobs + command patch) + ciip_pred_kernel, against (b) the two vvc355_bipred_batch
           launches (luma jobs, chroma jobs) of the host-built path on the same jobs; the builder alone is listed too.  Device events
           around each piece, the pieces alternating in one process, median per round, median of the rounds.
Both paths must leave identical scratch buffers (and the device's job array must equal the host-built one) before anything is timed.
A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/ciip_frame_time.py [--reps 100] [--rounds 5] [--out profiles/ciip_frame_pass.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INTER_FRAC, CIIP_FRAC, CTB = 0.8, 0.02, 128          # bench.py's CTU kinds


def clock_state():
    """The clocks as the driver reports them (read only), before and after the timed loops."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, timeout=60, text=True)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr[-200:]}
    except Exception as e:                    # no tool, no permission: say so in the profile instead of failing the measurement
        return {"unavailable": repr(e)}


def bench_population(width, height):
    """recon_cases.ReconWork as bench.py builds it for a picture of this size (build_chain: the same generators and draws)."""
    import recon_cases
    ncx, ncy = (width + CTB - 1) // CTB, (height + CTB - 1) // CTB
    rng = np.random.default_rng(0x5EED0001)
    ctu_inter = rng.random(ncx * ncy) < INTER_FRAC
    ctu_ciip = ctu_inter & (rng.random(ncx * ncy) < CIIP_FRAC / INTER_FRAC)
    in_order = (~ctu_inter | ctu_ciip).reshape(ncy, ncx)
    nb = np.zeros_like(in_order)
    nb[:, 1:] |= in_order[:, :-1]
    nb[1:, :] |= in_order[:-1, :]
    ctu_dep = ctu_inter & ~ctu_ciip & nb.reshape(-1)
    return recon_cases.ReconWork(np.random.default_rng(0x5EED0EC0), width, height, 7, 1, 1, intra_ctu=~ctu_inter, split=(0.6, 0.1), ciip_ctu=ctu_ciip,
                                 lmcs=True, resid_ctu=ctu_dep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every piece in every round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds; the spread is taken over the rounds' medians")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ciip_frame_pass.json"))
    args = ap.parse_args()

    import torch
    import bipred_cases as bc
    import ciip_frame_cases as cc
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ciip_frame_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    bd, isz = args.bd, 1 if args.bd == 8 else 2
    width, height = args.width, args.height

    # ---- the picture: bench.py's CIIP units, one record each, the MvField entries they read, one slice with LMCS
    work = bench_population(width, height)
    p = cc.CiipPicture(width, height, 7, 1, isz)
    p.slice_idx, p.col_bd, p.row_bd = work.slice_idx, work.col_bd, work.row_bd
    p.slices = (abi.InterSlice * 2)()
    p.slices[0].lmcs_used = 1
    rng = np.random.default_rng(0x5EED0C11)
    units, named = [], []
    for (c, x, y, w, h, off, k) in work.ciip:
        if c == 0:
            blk = p.mvf[y // 4:(y + h) // 4, x // 4:(x + w) // 4]
            blk["mv"], blk["ref_idx"], blk["pred_flag"], blk["ciip_flag"] = rng.integers(-24 * 16, 24 * 16 + 1, size=(2, 2)), [0, 0], 3, 1
            units.append((x, y, w, h, 0, 0, off))
            named.append([cc.NO_CMD] * 3)
        named[-1][c] = k
    if not units:
        sys.exit("ciip_frame_time: the picture has no CIIP unit")
    p.set_records(rng, [u[:6] for u in units], gaps=False)
    p.cus["scratch_off"] = [u[6] for u in units]
    p.cus["cmd"] = named
    p.scratch_len = work.ciip_len
    p.cmds = work.bind(0, 0, isz)
    is_ciip = p.cmds["kind"] == abi.RECON_CIIP
    p.cmds["resid"][is_ciip] = 0
    p.cmds["joint"][is_ciip] = 0

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    dims = [(width, height), (width >> 1, height >> 1), (width >> 1, height >> 1)]
    pitches = [batch.plane_pitch(d[0], isz) for d in dims]
    prng = np.random.default_rng(0x5EED0C12)
    base = [bc.smooth_picture(prng, ph, pw, bd, scale=32) for (pw, ph) in dims]
    refs = [[base[c], bc.shifted(base[c], 2 >> (c > 0), -2 >> (c > 0))][r] for r in range(2) for c in range(3)]
    d_ref = [on_device(batch.to_pitched(a)) for a in refs]                     # [list * 3 + component]: one reference picture per list
    d_dst = [torch.zeros(dims[c][1] * pitches[c], dtype=torch.uint8, device="cuda") for c in range(3)]
    lut = np.sort(np.random.default_rng(0x5EED0ECF).integers(0, 1 << bd, size=1 << bd)).astype(base[0].dtype)
    t_refs = (abi.RefPic * 32)()
    for l in range(2):
        for c in range(3):
            t_refs[l * 16].plane[c], t_refs[l * 16].stride[c] = d_ref[l * 3 + c].data_ptr(), pitches[c]
    d_reft, d_mvf, d_sl, d_lut = (on_device(a) for a in (np.frombuffer(bytes(t_refs), np.uint8), p.mvf, np.frombuffer(bytes(p.slices), np.uint8), lut))
    d_cus, d_cmds = on_device(p.cus), on_device(p.cmds)
    d_tabs = [on_device(a) for a in (p.slice_idx, p.col_bd, p.row_bd)]
    d_jobs = torch.zeros(p.n_jobs * cc.BIPRED_JOB_DT.itemsize, dtype=torch.uint8, device="cuda")
    scratch_a = torch.full((p.scratch_len * isz,), 0xEE, dtype=torch.uint8, device="cuda")
    scratch_b = torch.full((p.scratch_len * isz,), 0xEE, dtype=torch.uint8, device="cuda")

    pic = p.pic([t.data_ptr() for t in d_dst], pitches, d_mvf.data_ptr(), d_reft.data_ptr(), d_sl.data_ptr(), d_lut.data_ptr())
    frame = p.frame(pic, d_cus.data_ptr(), d_jobs.data_ptr(), scratch_a.data_ptr(), d_cmds.data_ptr(), *(t.data_ptr() for t in d_tabs))
    d_frame = on_device(np.frombuffer(bytes(frame), np.uint8))

    # ---- the host-built path: the same jobs (the numpy restatement), luma and chroma arrays as bench.py uploads them
    def host_jobs(scratch_ptr):
        return cc.expect_jobs(p, lambda c: (d_dst[c].data_ptr(), pitches[c]), lambda l, r, c: (d_ref[l * 3 + c].data_ptr(), pitches[c]), scratch_ptr, d_lut.data_ptr())

    jobs_b = host_jobs(scratch_b.data_ptr())
    jl, jc = jobs_b[jobs_b["chroma"] == 0], jobs_b[jobs_b["chroma"] != 0]
    d_jl, d_jc = on_device(jl), on_device(jc)

    def records_path():
        assert dev.vvc355_ciip_frame_pass(st, bd, d_frame.data_ptr(), ctypes.addressof(frame)) == 0

    def builder_alone():
        assert dev.vvc355_ciip_frame_build(st, d_frame.data_ptr(), ctypes.addressof(frame)) == 0

    def host_path():
        dev.vvc355_bipred_batch(st, bd, d_jl.data_ptr(), len(jl))
        dev.vvc355_bipred_batch(st, bd, d_jc.data_ptr(), len(jc))

    pieces = {"a_builder_and_ciip_pred": records_path, "b_two_bipred_batches": host_path, "builder_alone": builder_alone}
    for launch in pieces.values():
        launch()
    torch.cuda.synchronize()
    if dev.vvc355_last_error() != 0:
        sys.exit("ciip_frame_time: a launch failed")
    got_jobs = d_jobs.cpu().numpy().view(cc.BIPRED_JOB_DT)
    jobs_equal = all(np.array_equal(got_jobs[n], host_jobs(scratch_a.data_ptr())[n]) for n in cc.BIPRED_JOB_DT.names)
    sa, sb = scratch_a.cpu().numpy(), scratch_b.cpu().numpy()
    scratch_equal = bool(np.array_equal(sa, sb)) and bool((sa.view(base[0].dtype) != (0xEEEE if isz == 2 else 0xEE)).mean() > 0.9)
    cmds_after = d_cmds.cpu().numpy().view(cc.CMD)
    cmds_equal = bool(np.array_equal(cmds_after, cc.expect_cmds(p, scratch_a.data_ptr())))
    if not (jobs_equal and scratch_equal and cmds_equal):
        sys.exit(f"ciip_frame_time: the two paths differ (jobs equal {jobs_equal}, scratch equal {scratch_equal}, commands as expected {cmds_equal}); nothing timed")

    clocks = [clock_state()]
    for _ in range(args.warmup):
        for launch in pieces.values():
            launch()
    torch.cuda.synchronize()
    rounds = {name: [] for name in pieces}
    for _r in range(args.rounds):
        ev = {name: [] for name in pieces}
        for _i in range(args.reps):
            for name, launch in pieces.items():                 # alternating
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                ev[name].append((a, b))
        torch.cuda.synchronize()
        for name in pieces:
            rounds[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[name]])))
    clocks.append(clock_state())

    def stat(v):
        v = np.array(v)
        return {"median_us": float(np.median(v)), "round_medians_us": [round(float(x), 2) for x in v], "spread_us": float(v.max() - v.min())}

    t = {name: stat(v) for name, v in rounds.items()}
    out = {
        "tool": "tools/ciip_frame_time.py", "device": torch.cuda.get_device_name(0),
        "picture": f"{width}x{height}", "bit_depth": bd, "what": "bench.py's CIIP population (recon_cases.ReconWork with its ciip_ctu mask), 4:2:0, CTU 128, LMCS on",
        "ciip_units": len(p.cus), "jobs": {"all": int(p.n_jobs), "luma": int(len(jl)), "chroma": int(len(jc))}, "ciip_commands": int(is_ciip.sum()),
        "both_paths_leave_identical_scratch": scratch_equal, "device_jobs_equal_host_built": jobs_equal, "commands_patched_as_expected": cmds_equal,
        "upload_bytes": {"a_records": int(p.cus.nbytes), "b_host_built_jobs": int(jobs_b.nbytes),
                         "note": "computed: 32 bytes per unit against 104 bytes per tile; the command array is uploaded either way"},
        "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median of the rounds",
        "repetitions_per_round": args.reps, "rounds": args.rounds,
        "time": t,
        "a_not_slower_than_b": bool(t["a_builder_and_ciip_pred"]["median_us"] <= t["b_two_bipred_batches"]["median_us"]),
        "clock_state": {"before": clocks[0], "after": clocks[1]},
    }
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

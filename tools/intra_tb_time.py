"""Times the intra transform stage of the bench's 8K 10-bit picture three ways, in one process, alternating:
  (a) the path vvc355_intra_tb_pass replaces, on packed levels: vvc355_levels_expand of the LFNST blocks + vvc355_lfnst_batch + one
      vvc355_itx_batch_lv per area class, from host-built 48-byte jobs and 32-byte LFNST jobs;
  (b) vvc355_intra_tb_pass, one launch per class (launch_mode 1);
  (c) vvc355_intra_tb_pass, classes 0-3 in one grid (launch_mode 2).
The population restates bench.py's: the CTU kinds of build_chain (80 % inter, CIIP, the inter CTUs whose chroma residuals the in-order pass
adds), recon_cases.ReconWork with the bench's arguments, then the LFNST fraction and window draws of its intra transform stage
(tests/intra_tb_cases.picture_specs).  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/intra_tb_time.py [--reps 200] [--rounds 5] [--out profiles/intra_tb_pass.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INTER_FRAC, CIIP_FRAC = 0.8, 0.02           # bench.py's CTU kinds


def population(width, height, seed):
    import intra_tb_cases as tc
    import recon_cases
    ncx, ncy = (width + 127) // 128, (height + 127) // 128
    rng = np.random.default_rng(seed)
    ctu_inter = rng.random(ncx * ncy) < INTER_FRAC
    ctu_ciip = ctu_inter & (rng.random(ncx * ncy) < CIIP_FRAC / INTER_FRAC)
    in_order = (~ctu_inter | ctu_ciip).reshape(ncy, ncx)
    nb = np.zeros_like(in_order)
    nb[:, 1:] |= in_order[:, :-1]
    nb[1:, :] |= in_order[:-1, :]
    ctu_dep = ctu_inter & ~ctu_ciip & nb.reshape(-1)
    work = recon_cases.ReconWork(np.random.default_rng(0x5EED0EC0), width, height, 7, 1, 1, intra_ctu=~ctu_inter, split=(0.6, 0.1),
                                 ciip_ctu=ctu_ciip, lmcs=True, resid_ctu=ctu_dep)
    return tc.picture_specs(np.random.default_rng(0x5EED0EC1), work.tbs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200, help="timed repetitions of every path (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_tb_pass.json"))
    args = ap.parse_args()

    import torch
    import intra_tb_cases as tc
    import levels_cases as lc
    from ffvvc_amd import abi
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("intra_tb_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    bd = args.bd

    specs, class_first = tc.group_by_class(population(args.width, args.height, 0x5EED0001))
    offs, n = tc.arena_offsets(specs)
    n_lf = sum(s["lfnst"] for s in specs)
    levels, lv = lc.pack_all([s["c"] for s in specs], force_int32={i for i in range(len(specs)) if i % 10 == 7})
    arena0 = tc.start_arena(specs, offs, n, lv)
    paths = {
        "a_expand_lfnst_itx_lv": tc.OldPath(specs, class_first, offs, arena0, bd, 15, (levels, lv)),
        "b_intra_tb_pass_per_class": tc.Frame(specs, class_first, offs, arena0, bd, 15, (levels, lv), 1),
        "c_intra_tb_pass_merged": tc.Frame(specs, class_first, offs, arena0, bd, 15, (levels, lv), 2),
    }
    d_arena0 = torch.from_numpy(arena0).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def restore(p):
        dev.vvc355_copy_async(st, p.d_arena.ptr, d_arena0.data_ptr(), arena0.nbytes)

    # identical results first (this also warms every launch shape once)
    arenas = {}
    for name, p in paths.items():
        restore(p)
        assert p.launch(dev, st) == 0
        torch.cuda.synchronize()
        arenas[name] = p.result(dev)
    names = list(paths)
    identical = all(np.array_equal(arenas[names[0]], arenas[k]) for k in names[1:])
    changed = int((arenas[names[0]] != arena0).sum())
    for _ in range(args.warmup):
        for p in paths.values():
            restore(p)
            p.launch(dev, st)
    torch.cuda.synchronize()

    per_round = max(1, args.reps // args.rounds)
    rounds = {k: [] for k in paths}
    for _r in range(args.rounds):
        ev = {k: [] for k in paths}
        for _i in range(per_round):
            for name, p in paths.items():              # alternating: a, b, c, a, b, c, ...
                restore(p)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                p.launch(dev, st)
                e1.record()
                ev[name].append((e0, e1))
        torch.cuda.synchronize()
        for name in paths:
            rounds[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[name]])))

    # the bytes the stage has to move, whatever the path: packed groups and side records in (int32 levels for the blocks that stay
    # unpacked), 16-byte records in, int32 residuals out
    samples = sum(s["c"].size for s in specs)
    int32_in = sum(s["c"].size * 4 for i, s in enumerate(specs) if lv[i]["flags"])
    alg_bytes = (len(levels) - 16) * 2 + len(specs) * (16 + 16) + int32_in + samples * 4
    out = {
        "tool": "tools/intra_tb_time.py", "picture": f"{args.width}x{args.height} {bd}-bit", "device": torch.cuda.get_device_name(0),
        "blocks": len(specs), "class_first": class_first, "lfnst_blocks": int(n_lf), "packed_fraction": float((lv["flags"] == 0).mean()),
        "residual_samples": int(samples), "algorithmic_bytes": int(alg_bytes),
        "repetitions_per_path": per_round * args.rounds, "rounds": args.rounds,
        "identical_arenas": bool(identical), "arena_words_written": changed,
        "upload_bytes_per_picture": {"jobs_48B_plus_lfnst_32B": int(len(specs) * 48 + n_lf * 32), "records_16B": int(len(specs) * 16)},
        "paths": {},
    }
    for name in paths:
        r = np.array(rounds[name])
        out["paths"][name] = {"median_us": float(np.median(r)), "round_medians_us": [round(float(v), 2) for v in r],
                              "spread_us": float(r.max() - r.min()), "algorithmic_GBps": float(alg_bytes / (np.median(r) * 1e-6) / 1e9)}
    print(json.dumps(out, indent=1))
    if not identical:
        sys.exit("intra_tb_time: the three paths do NOT produce identical arenas")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

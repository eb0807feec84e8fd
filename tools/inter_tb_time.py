"""Times the transform stage of the inter coding units of the bench's 8K 10-bit picture two ways, in one process, alternating:
  old  vvc355_itx_frame_build (48-byte jobs + 56-byte residual jobs into device scratch) + one vvc355_itx_shape_batch_lv per shape +
       vvc355_lmcs_chroma_resid_batch over every slot;
  new  vvc355_inter_tb_pass(luma) + vvc355_inter_tb_pass(chroma) from the same blocks as 16-byte vvc355_inter_tu records.
vvc355_lmcs_vpdu_scale_pass sits between the luma and the chroma work of both and is timed on its own.  Every piece is timed with events
around it inside a whole run of its path (build, shapes, scale, resid / luma, scale, chroma), so each works on the state the pieces before
it left.  The population restates bench.py's: the CTU kinds of build_chain (80 % inter, CIIP, the inter CTUs whose chroma residuals the
in-order pass adds), then per inter CTU one 64x64, four 32x32, sixteen 16x16 and sixty-four 8x8 luma blocks and per chroma component one
32x32, four 16x16, sixteen 8x8 and sixty-four 4x4 blocks, windows and levels as the bench draws them, LMCS on, packed levels.  Luma blocks
of 4..32 take DST-7 / DCT-8 pairs on 30 % of the blocks through explicit mts_idx (the bench sets trh / trv directly); chroma is DCT-2, as
the syntax has it.  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/inter_tb_time.py [--reps 100] [--rounds 5] [--out profiles/inter_tb_pass.json]
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
CTB = 128


def population(width, height, seed):
    """The specs of tests/inter_tb_cases.py for the bench's inter transform blocks."""
    import inter_tb_cases as tc
    import levels_cases as lc
    from ffvvc_amd import abi
    ncx, ncy = (width + CTB - 1) // CTB, (height + CTB - 1) // CTB
    rng = np.random.default_rng(seed)
    ctu_inter = rng.random(ncx * ncy) < INTER_FRAC
    ctu_ciip = ctu_inter & (rng.random(ncx * ncy) < CIIP_FRAC / INTER_FRAC)
    in_order = (~ctu_inter | ctu_ciip).reshape(ncy, ncx)
    nb = np.zeros_like(in_order)
    nb[:, 1:] |= in_order[:, :-1]
    nb[1:, :] |= in_order[:-1, :]
    ctu_dep = ctu_inter & ~ctu_ciip & nb.reshape(-1)
    specs = []
    for c in range(3):
        cs = CTB if c == 0 else CTB // 2
        parts = [(0, 0, 64), (64, 0, 32), (0, 64, 16), (64, 64, 8)] if c == 0 else [(0, 0, 32), (32, 0, 16), (0, 32, 8), (32, 32, 4)]
        for ry in range(height // CTB):
            for rx in range(width // CTB):
                k = ry * ncx + rx
                if not ctu_inter[k] or ctu_ciip[k] or (c and ctu_dep[k]):
                    continue
                for (qx, qy, n) in parts:
                    lg = n.bit_length() - 1
                    for oy in range(0, cs // 2, n):
                        for ox in range(0, cs // 2, n):
                            mts = int(rng.integers(1, 5)) if (c == 0 and 4 <= n <= 32 and rng.random() < 0.3) else 0
                            lim = min(16 if mts else 32, n)
                            nzw, nzh = 1 + int(rng.random() * lim), 1 + int(rng.random() * lim)
                            blk = np.zeros((n, n), np.int32)
                            blk[:nzh, :nzw] = lc.laplace_levels(rng, (nzh, nzw))
                            specs.append(tc.spec(c, rx * cs + qx + ox, ry * cs + qy + oy, lg, lg, blk, nzw, nzh, qp=int(rng.integers(22, 38)),
                                                 dep=int(rng.integers(0, 2)), tu_flags=abi.TU_MTS_ENABLED, mts_idx=mts, joint=8 if c else 0))
    return specs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every path (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inter_tb_pass.json"))
    args = ap.parse_args()

    import torch
    import inter_tb_cases as tc
    import levels_cases as lc
    import recon_cases
    from conftest import load_oracle
    from ffvvc_amd import abi
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("inter_tb_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    orc = load_oracle()
    tc.bind_oracle(orc)
    bd = args.bd

    rng = np.random.default_rng(0x5EED0002)
    pic = tc.Picture.random(rng, bd, args.width, args.height)
    pic.model = recon_cases.ReconWork.lmcs_model(rng, bd)
    specs, bin_first = tc.group(population(args.width, args.height, 0x5EED0001))
    offs, n = tc.arena_offsets(specs)
    levels, lv = lc.pack_all([s["c"] for s in specs])
    arena0 = tc.start_arena(specs, offs, n, lv)
    new = tc.Frame(pic, specs, bin_first, offs, arena0, 15, (levels, lv))
    old = tc.OldPath(orc, pic, specs, offs, arena0, 15, (levels, lv))
    st = torch.cuda.current_stream().cuda_stream

    # pristine planes on the device, so that a restore is a device copy
    pristine = [torch.from_numpy(h.view(np.uint8).copy()).cuda() for h in new.dpic.host]

    def restore(p):
        for d, src in zip(p.dpic.d_planes, pristine):
            dev.vvc355_copy_async(st, d.ptr, src.data_ptr(), src.numel())

    pieces = {
        "old": [("itx_frame_build", lambda: old.build(dev, st)), ("shape_launches", lambda: old.shapes(dev, st)),
                ("lmcs_vpdu_scale_pass", lambda: old.dpic.scale_pass(dev, st)), ("lmcs_chroma_resid_batch", lambda: old.resid(dev, st))],
        "new": [("inter_tb_pass_luma", lambda: new.launch(dev, 1, st)), ("lmcs_vpdu_scale_pass", lambda: new.dpic.scale_pass(dev, st)),
                ("inter_tb_pass_chroma", lambda: new.launch(dev, 2, st))],
    }
    paths = {"old": old, "new": new}

    def run(name, timed=None):
        restore(paths[name])
        for piece, fn in pieces[name]:
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = fn()
            assert not rc, (name, piece, rc)
            if timed is not None:
                e1.record()
                timed[(name, piece)].append((e0, e1))

    # identical planes first (this also warms every launch shape once)
    planes = {}
    for name in paths:
        run(name)
        torch.cuda.synchronize()
        planes[name] = paths[name].dpic.pitched_planes(dev)
    identical = all(np.array_equal(a, b) for a, b in zip(planes["old"], planes["new"]))
    changed = [int((a != h).sum()) for a, h in zip(planes["new"], new.dpic.host)]
    for _ in range(args.warmup):
        for name in paths:
            run(name)
    torch.cuda.synchronize()

    per_round = max(1, args.reps // args.rounds)
    keys = [(name, piece) for name in pieces for piece, _ in pieces[name]]
    rounds = {k: [] for k in keys}
    for _r in range(args.rounds):
        ev = {k: [] for k in keys}
        for _i in range(per_round):
            for name in paths:                         # alternating: old, new, old, new, ...
                run(name, ev)
        torch.cuda.synchronize()
        for k in keys:
            rounds[k].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[k]])))

    def stat(ks):
        r = np.sum([rounds[k] for k in ks], axis=0)
        return {"median_us": float(np.median(r)), "round_medians_us": [round(float(v), 2) for v in r], "spread_us": float(r.max() - r.min())}

    n_chroma = sum(1 for s in specs if s["c_idx"])
    chroma_samples = sum(s["c"].size for s in specs if s["c_idx"])
    out = {
        "tool": "tools/inter_tb_time.py", "picture": f"{args.width}x{args.height} {bd}-bit", "device": torch.cuda.get_device_name(0),
        "blocks": len(specs), "chroma_blocks": n_chroma, "samples": int(sum(s["c"].size for s in specs)),
        "non_empty_bins": [[k for k in range(tc.NB) if bin_first[ch][k + 1] > bin_first[ch][k]] for ch in range(2)],
        "packed_fraction": float((lv["flags"] == 0).mean()),
        "repetitions_per_path": per_round * args.rounds, "rounds": args.rounds,
        "identical_planes": bool(identical), "samples_changed_per_plane": changed,
        "device_scratch_bytes": {"old_jobs_48B_plus_resid_jobs_56B": int(len(specs) * (48 + 56)), "new": 0},
        "arena_bytes_chroma_residuals": {"old_written_then_read_back": int(2 * 4 * chroma_samples), "new": 0},
        "pieces": {f"{name}.{piece}": stat([(name, piece)]) for (name, piece) in keys},
        "old_sum": stat([("old", "itx_frame_build"), ("old", "shape_launches"), ("old", "lmcs_chroma_resid_batch")]),
        "new_sum": stat([("new", "inter_tb_pass_luma"), ("new", "inter_tb_pass_chroma")]),
    }
    gap = out["old_sum"]["median_us"] - out["new_sum"]["median_us"]
    out["old_minus_new_us"] = gap
    out["faster_by_more_than_the_larger_spread"] = bool(gap > max(out["old_sum"]["spread_us"], out["new_sum"]["spread_us"]))
    print(json.dumps(out, indent=1))
    if not identical:
        sys.exit("inter_tb_time: the two paths do NOT leave identical planes")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

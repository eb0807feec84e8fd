"""Times the transform-skip blocks of an 8K 10-bit picture, in one process:
  old  vvc355_levels_expand (a 48-byte vvc355_itx_job per block for address and shape) + vvc355_dequant_batch (a 32-byte job per block,
       ts = 1): the only batched path the library had for these blocks, and it exists for KEEP blocks without BDPCM only;
  new  vvc355_ts_tb_pass (both channel types in one call) from the same blocks as 16-byte vvc355_ts_tu records.
The two alternate, after a check that they leave identical arenas; every piece sits between device events.  The BDPCM and the add variants
of the same blocks (KEEP + BDPCM, plain add, add + BDPCM; the directions alternate from block to block) have no batched predecessor: they
are timed in the same loop and reported without a comparison.  The add variants are not restored between repetitions (the samples clip,
the traffic is the same).

The population: every fourth CTU (128x128, at random) of the picture is coded with transform skip throughout.  Its luma quadrants hold four
32x32, sixteen 16x16, sixty-four 8x8 and 256 4x4 blocks, each chroma component's quadrants one 32x32, four 16x16, sixteen 8x8 and (the last)
thirty-two 4x4, sixteen 8x2 and sixteen 2x8 blocks; windows are uniform in 1..side per axis, levels Laplacian, qp 22..37, levels packed.
The counts per shape are written into the output.  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside
the repository.

    python tools/ts_tb_time.py [--reps 100] [--rounds 5] [--out profiles/ts_tb_pass.json]
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

TS_FRAC = 0.25
CTB = 128


def population(width, height, seed):
    """The specs of tests/ts_tb_cases.py for the picture's transform-skip blocks, all KEEP, no BDPCM."""
    import levels_cases as lc
    import ts_tb_cases as ts
    ncx = (width + CTB - 1) // CTB
    rng = np.random.default_rng(seed)
    ctu_ts = rng.random(ncx * ((height + CTB - 1) // CTB)) < TS_FRAC
    specs = []

    def block(c, x, y, lw, lh):
        w, h = 1 << lw, 1 << lh
        nzw, nzh = 1 + int(rng.random() * w), 1 + int(rng.random() * h)
        blk = np.zeros((h, w), np.int32)
        blk[:nzh, :nzw] = lc.laplace_levels(rng, (nzh, nzw))
        specs.append(ts.spec(c, x, y, lw, lh, blk, nzw, nzh, qp=int(rng.integers(22, 38)), keep=True))

    for c in range(3):
        cs = CTB if c == 0 else CTB // 2
        q = cs // 2
        for ry in range(height // CTB):
            for rx in range(width // CTB):
                if not ctu_ts[ry * ncx + rx]:
                    continue
                bx, by = rx * cs, ry * cs
                for k, (qx, qy) in enumerate([(0, 0), (q, 0), (0, q), (q, q)]):
                    n = (q >> 1) >> k                        # luma 32, 16, 8, 4; chroma 16, 8, 4, 2
                    if c == 0:
                        for oy in range(0, q, n):
                            for ox in range(0, q, n):
                                block(c, bx + qx + ox, by + qy + oy, n.bit_length() - 1, n.bit_length() - 1)
                        continue
                    n *= 2                                   # chroma: 32, 16, 8, then the mixed quadrant
                    if k < 3:
                        for oy in range(0, q, n):
                            for ox in range(0, q, n):
                                block(c, bx + qx + ox, by + qy + oy, n.bit_length() - 1, n.bit_length() - 1)
                        continue
                    for oy in range(0, 16, 4):               # 32 x 16 samples of 4x4
                        for ox in range(0, 32, 4):
                            block(c, bx + qx + ox, by + qy + oy, 2, 2)
                    for oy in range(16, 24, 2):              # 32 x 8 samples of 8x2
                        for ox in range(0, 32, 8):
                            block(c, bx + qx + ox, by + qy + oy, 3, 1)
                    for oy in range(24, 32, 8):              # 32 x 8 samples of 2x8
                        for ox in range(0, 32, 2):
                            block(c, bx + qx + ox, by + qy + oy, 1, 3)
    return specs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--bd", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every path (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ts_tb_pass.json"))
    args = ap.parse_args()

    import torch
    import inter_tb_cases as tc
    import levels_cases as lc
    import ts_tb_cases as ts
    from ffvvc_amd import abi, batch
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("ts_tb_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    bd = args.bd

    rng = np.random.default_rng(0x5EED0012)
    pic = tc.Picture.random(rng, bd, args.width, args.height)
    specs, class_first = ts.group(population(args.width, args.height, 0x5EED0011))
    offs, n = tc.arena_offsets(specs)
    levels, lv = lc.pack_all([s["c"] for s in specs])
    assert not lv["flags"].any()
    arena0 = tc.start_arena(specs, offs, n, lv)
    keep = ts.Frame(pic, specs, class_first, offs, arena0, 15, (levels, lv))
    old = ts.OldPath(pic, specs, offs, arena0, 15, (levels, lv))
    st = torch.cuda.current_stream().cuda_stream

    class Variant:
        """The same blocks, arena, levels and picture with other record flags."""

        def __init__(self, clear, bdpcm):
            tus = ts.records(pic, specs, offs)
            tus["flags"] &= ~np.uint8(clear)
            if bdpcm:
                tus["flags"] |= np.uint8(abi.TS_TU_BDPCM)
                tus["flags"][1::2] |= np.uint8(abi.TS_TU_VERTICAL)
            self.d_tus = batch.DeviceBuffer.from_host(tus.view(np.uint8))
            self.f = abi.TsTbFrame.from_buffer_copy(bytes(keep.f))
            self.f.tus = self.d_tus.ptr
            self.d_f = batch.DeviceBuffer.from_host(np.frombuffer(bytes(self.f), np.uint8))

        def launch(self):
            return dev.vvc355_ts_tb_pass(st, self.d_f.ptr, ctypes.addressof(self.f), 3)

    variants = {"keep_bdpcm": Variant(0, True), "add": Variant(abi.TS_TU_KEEP, False), "add_bdpcm": Variant(abi.TS_TU_KEEP, True)}
    pieces = [("old", "levels_expand", lambda: old.expand(dev, st)), ("old", "dequant_batch", lambda: old.dequant(dev, st)),
              ("new", "ts_tb_pass", lambda: keep.launch(dev, 3, st))]
    pieces += [(name, "ts_tb_pass", v.launch) for name, v in variants.items()]

    def run(timed=None):
        for name, piece, fn in pieces:                       # alternating: old, new, variants, old, new, ...
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            rc = fn()
            assert not rc, (name, piece, rc)
            if timed is not None:
                e1.record()
                timed[(name, piece)].append((e0, e1))

    # identical arenas first, before any variant has written to the new path's arena (this also warms the launches)
    for _name, _piece, fn in pieces[:3]:
        assert not fn()
    torch.cuda.synchronize()
    a_old, a_new = old.arena(dev), keep.arena(dev)
    identical = bool(np.array_equal(a_old, a_new))
    changed = int((a_new != arena0).sum())
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()

    per_round = max(1, args.reps // args.rounds)
    keys = [(name, piece) for name, piece, _ in pieces]
    rounds = {k: [] for k in keys}
    for _r in range(args.rounds):
        ev = {k: [] for k in keys}
        for _i in range(per_round):
            run(ev)
        torch.cuda.synchronize()
        for k in keys:
            rounds[k].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[k]])))

    def stat(ks):
        r = np.sum([rounds[k] for k in ks], axis=0)
        return {"median_us": float(np.median(r)), "round_medians_us": [round(float(v), 2) for v in r], "spread_us": float(r.max() - r.min())}

    shapes = {}
    for s in specs:
        key = f"{'luma' if s['c_idx'] == 0 else 'chroma'} {1 << s['lw']}x{1 << s['lh']}"
        shapes[key] = shapes.get(key, 0) + 1
    samples = int(sum(s["c"].size for s in specs))
    window = int(sum(s["nzw"] * s["nzh"] for s in specs))
    out = {
        "tool": "tools/ts_tb_time.py", "picture": f"{args.width}x{args.height} {bd}-bit", "device": torch.cuda.get_device_name(0),
        "population": {"ctu_fraction": TS_FRAC, "blocks": len(specs), "blocks_per_shape": shapes, "samples": samples,
                       "samples_inside_level_windows": window, "level_groups_32B": int(len(levels) // 16),
                       "class_first": class_first, "packed_fraction": float((lv["flags"] == 0).mean())},
        "repetitions_per_path": per_round * args.rounds, "rounds": args.rounds,
        "identical_arenas": identical, "arena_words_changed": changed,
        "device_job_bytes": {"old_itx_jobs_48B_plus_dequant_jobs_32B": int(old.job_bytes), "new_records_16B": int(16 * len(specs))},
        "pieces": {f"{name}.{piece}": stat([(name, piece)]) for (name, piece) in keys},
        "old_sum": stat([("old", "levels_expand"), ("old", "dequant_batch")]),
        "new": stat([("new", "ts_tb_pass")]),
    }
    gap = out["old_sum"]["median_us"] - out["new"]["median_us"]
    out["old_minus_new_us"] = gap
    out["new_not_above_old_plus_spread"] = bool(out["new"]["median_us"] <= out["old_sum"]["median_us"] + min(out["old_sum"]["spread_us"], out["new"]["spread_us"]))
    out["faster_by_more_than_the_larger_spread"] = bool(gap > max(out["old_sum"]["spread_us"], out["new"]["spread_us"]))
    print(json.dumps(out, indent=1))
    if not identical:
        sys.exit("ts_tb_time: the two paths do NOT leave identical arenas")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

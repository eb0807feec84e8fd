"""What vvc355_mvf_unit_pass costs and saves next to the path it replaces (the host derives the field of affine and GPM units, cuts it into
rectangles of equal motion and vvc355_tab_fill_pass paints them), on two 8K pictures (7680x4320, CTU 128).  Both take the coding units of
the bench's partition (bs_cases.BsTables with the bench's seed and split, a quarter-width picture repeated four times across):
  bench   the bench's unit statistics: its affine-flagged coding units become AFFINE records (where both sides are powers of two), its
          sub-block-merge units 8x8 PLAIN records, everything else one PLAIN record (intra units: the zero MvField);
  third   coding units turned AFFINE until a third of the picture's area is, and a twentieth GPM.
Per picture:
  bytes    what a caller uploads: 64 bytes per unit record against 32 per rectangle of equal motion (one per 4x4 block of an AFFINE or GPM
           unit, one per unit where the whole unit came out with one motion).  Computed from the record counts, not measured.
  kernel   vvc355_mvf_unit_pass alone against vvc355_tab_fill_pass with the motion records only, each between device events of its own,
           alternating inside every repetition, median per round, median of the rounds.
  h2d      the pinned host-to-device copy of either record array followed by its kernel, measured the same way.
The device's table and affine records must equal the numpy side's (mvf_unit_cases) before anything is timed, and the table the parent's
path writes must equal it too.  A tool, not a test: it needs an MI355X and fails without one; it reads nothing outside the repository.

    python tools/mvf_unit_time.py [--reps 100] [--rounds 5] [--out profiles/mvf_unit.json]
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

WIDTH, HEIGHT, REPS_X = 7680, 4320, 4


def clock_state():
    """The clocks as the driver reports them (read only), before and after the timed loops."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--json"], capture_output=True, timeout=60, text=True)
        return json.loads(r.stdout) if r.returncode == 0 else {"unavailable": r.stderr[-200:]}
    except Exception as e:                    # no tool, no permission: say so in the profile instead of failing the measurement
        return {"unavailable": repr(e)}


def quarter_units(mc, bt, mode, rng):
    """The unit records of the quarter-width picture `bt` (see the module's text): (records, number of AFFINE records, area fractions)."""
    leaves = [(x, y, w, h, bool(bt.mvf[y // 4, x // 4]["pred_flag"]), bool(bt.iaf[y // 4, x // 4]), bool(bt.msf[y // 4, x // 4]))
              for (x, y, w, h, _, _) in bt.cu_recs]
    total = float(bt.width * bt.height)
    pow2 = lambda w, h: not (w & (w - 1)) and not (h & (h - 1))          # noqa: E731
    want_aff = want_gpm = set()
    if mode == "third":
        order = rng.permutation(len(leaves))
        want_aff, want_gpm, a_aff, a_gpm = set(), set(), 0.0, 0.0
        for i in order:
            x, y, w, h, inter, _, _ = leaves[i]
            if a_aff < total / 3 and pow2(w, h):
                want_aff.add(i)
                a_aff += w * h
            elif a_gpm < total / 20 and (w, h) in mc.GPM_SHAPES:
                want_gpm.add(i)
                a_gpm += w * h
    units, n_aff, area = [], 0, {"affine": 0.0, "gpm": 0.0, "sub_block_merge": 0.0}
    for i, (x, y, w, h, inter, iaf, msf) in enumerate(leaves):
        as_aff = (i in want_aff) if mode == "third" else (inter and iaf and pow2(w, h))
        if as_aff:
            model, pred = int(rng.integers(1, 3)), int(rng.integers(1, 4))
            cp = mc.rand_cp(rng, "small" if rng.random() < 0.9 else "fallback", w, h, model)
            units.append(mc.affine(x, y, w, h, model, pred, cp, [int(rng.integers(0, 3)) if pred >> l & 1 else -1 for l in range(2)], 0, 0, link=n_aff))
            n_aff += 1
            area["affine"] += w * h
        elif i in want_gpm:
            units.append(mc.gpm(x, y, w, h, int(rng.integers(0, 64)), mc.rand_mvfield(rng, int(rng.integers(1, 3))), mc.rand_mvfield(rng, int(rng.integers(1, 3)))))
            area["gpm"] += w * h
        elif inter and (msf or iaf) and mode == "bench":
            units += [mc.plain(x + bx, y + by, 8, 8, mc.rand_mvfield(rng)) for by in range(0, h, 8) for bx in range(0, w, 8)]
            area["sub_block_merge"] += w * h
        else:
            units.append(mc.plain(x, y, w, h, mc.rand_mvfield(rng) if inter else mc.mvfield()))
    return np.array(units, mc.UNIT_DT), n_aff, {k: v / total for k, v in area.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of every piece (split over the rounds)")
    ap.add_argument("--rounds", type=int, default=5, help="rounds the repetitions are split into; the spread is taken over the rounds")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvf_unit.json"))
    args = ap.parse_args()

    import torch
    import bs_cases
    import mvf_unit_cases as mc
    from ffvvc_amd import abi
    dev = abi.load()
    if dev.vvc355_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("mvf_unit_time: no MI355X visible; this tool measures on the GPU and has no other mode")
    dev.vvc355_set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    qw = WIDTH // REPS_X
    bt = bs_cases.BsTables(np.random.default_rng(0x5EED0B5), qw, HEIGHT, 7, split=(0.95, 0.45), cbf_p=0.4)
    g, gq = mc.Geo(WIDTH, HEIGHT, 7), mc.Geo(qw, HEIGHT, 7)

    def on_device(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def pinned(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).pin_memory()

    def measure(mode):
        rng = np.random.default_rng(mc.SEED + 5000 + len(mode))
        q_units, q_aff, area = quarter_units(mc, bt, mode, rng)
        q_units, q_first = mc.group(gq, q_units)
        # the numpy side on the quarter picture; the full picture is the quarter four times across
        q_table, q_cus = np.zeros((gq.th, gq.tw), mc.MVF_DT), mc.sentinel_cus(q_aff)
        placed = mc.expect_table(gq, q_units, q_first, q_table, q_aff)
        assert placed.all()
        mc.expect_affine_cus(gq, q_units, q_first, q_cus)
        q_recs, _ = mc.expand(gq, q_units, q_first, q_aff)
        parts, rparts = [], []
        for k in range(REPS_X):
            u, r = q_units.copy(), q_recs.copy()
            u["x0"] += k * qw
            r["x0"] += k * qw
            aff = u["kind"] == mc.AFFINE
            u["link"][aff] += k * q_aff
            parts.append(u)
            rparts.append(r)
        units, first = mc.group(g, np.concatenate(parts))
        recs = np.concatenate(rparts)
        rs = (recs["y0"].astype(np.int64) >> 7) * g.cw + (recs["x0"].astype(np.int64) >> 7)
        order = np.argsort(rs, kind="stable")
        recs, rfirst = np.ascontiguousarray(recs[order]), np.searchsorted(rs[order], np.arange(g.cw * g.ch + 1)).astype(np.int32)
        want, want_cus = np.tile(q_table, (1, REPS_X)), np.tile(q_cus, REPS_X)
        n_aff = q_aff * REPS_X

        d_units, d_first, d_recs, d_rfirst = on_device(units), on_device(first), on_device(recs), on_device(rfirst)
        h_units, h_recs = pinned(units), pinned(recs)
        d_tab = [torch.full((g.th * g.tw * 24,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_cus = on_device(mc.sentinel_cus(max(1, n_aff)))
        uf = mc.unit_frame(g, d_units.data_ptr(), len(units), d_first.data_ptr(), d_tab[0].data_ptr(), g.tw, d_cus.data_ptr() if n_aff else 0, n_aff)
        tf = abi.TabFill()
        tf.mv, tf.n_mv, tf.ctu_first_mv, tf.mvf, tf.mvf_pitch, tf.unit_pitch = d_recs.data_ptr(), len(recs), d_rfirst.data_ptr(), d_tab[1].data_ptr(), g.tw, g.tw
        tf.ctb_log2, tf.width, tf.height, tf.ctb_width, tf.ctb_height, tf.hs, tf.vs = 7, g.width, g.height, g.cw, g.ch, 1, 1
        d_uf, d_tf = on_device(np.frombuffer(bytes(uf), np.uint8)), on_device(np.frombuffer(bytes(tf), np.uint8))

        def unit_pass():
            assert dev.vvc355_mvf_unit_pass(st, d_uf.data_ptr(), ctypes.addressof(uf)) == 0

        def tab_fill():
            dev.vvc355_tab_fill_pass(st, d_tf.data_ptr(), ctypes.addressof(tf))

        def units_h2d_and_pass():
            d_units.copy_(h_units, non_blocking=True)
            unit_pass()

        def recs_h2d_and_tab_fill():
            d_recs.copy_(h_recs, non_blocking=True)
            tab_fill()

        pieces = {"mvf_unit_pass": unit_pass, "tab_fill_pass_motion_only": tab_fill, "b_units_h2d_and_pass": units_h2d_and_pass,
                  "a_mv_recs_h2d_and_tab_fill": recs_h2d_and_tab_fill}
        for launch in pieces.values():
            launch()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().view(mc.MVF_DT).reshape(g.th, g.tw) for t in d_tab]
        differing = [n for n, t in zip(("mvf_unit_pass", "tab_fill_pass"), got) if mc.table_mismatch(t, want)]
        if n_aff and mc.cus_mismatch(d_cus.cpu().numpy().view(mc.CU_DT), want_cus):
            differing.append("affine_cus")
        for _ in range(args.warmup):
            for launch in pieces.values():
                launch()
        torch.cuda.synchronize()
        per_round = max(1, args.reps // args.rounds)
        rounds = {name: [] for name in pieces}
        for _r in range(args.rounds):
            ev = {name: [] for name in pieces}
            for _i in range(per_round):
                for name, launch in pieces.items():                 # alternating
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    launch()
                    b.record()
                    ev[name].append((a, b))
            torch.cuda.synchronize()
            for name in pieces:
                rounds[name].append(float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev[name]])))

        def stat(v):
            v = np.array(v)
            return {"median_us": float(np.median(v)), "round_medians_us": [round(float(x), 2) for x in v], "spread_us": float(v.max() - v.min())}

        kinds = np.bincount(units["kind"], minlength=3)
        out = {
            "picture": f"{WIDTH}x{HEIGHT}", "what": mode, "ctus": int(g.cw * g.ch), "area_fraction": area,
            "unit_records": {"plain": int(kinds[0]), "affine": int(kinds[1]), "gpm": int(kinds[2]), "total": int(len(units))},
            "mv_recs_of_the_parents_path": int(len(recs)),
            "outputs_equal_the_numpy_side": not differing, "differing": differing,
            "upload_bytes": {"a_mv_recs": int(recs.nbytes), "b_unit_records": int(units.nbytes), "ctu_first_either_way": int(first.nbytes),
                             "note": "computed from the record counts; vvc355_affine_cu (144 bytes per affine unit) travels either way, with "
                                     "prof_flags and diff_mv filled on the host only in (a)"},
            "repetitions_per_piece": per_round * args.rounds, "rounds": args.rounds,
            "kernel": {n: stat(rounds[n]) for n in ("mvf_unit_pass", "tab_fill_pass_motion_only")},
            "h2d": {n: stat(rounds[n]) for n in ("a_mv_recs_h2d_and_tab_fill", "b_units_h2d_and_pass")},
        }
        k = out["kernel"]
        out["kernel"]["mvf_unit_pass_not_slower_than_tab_fill"] = bool(k["mvf_unit_pass"]["median_us"] <= k["tab_fill_pass_motion_only"]["median_us"])
        return out, differing

    clocks = [clock_state()]
    results, failed = [], []
    for mode in ("bench", "third"):
        r, differing = measure(mode)
        results.append(r)
        failed += differing
    clocks.append(clock_state())
    out = {"tool": "tools/mvf_unit_time.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around each piece, pieces alternating inside every repetition, median per round, median of the rounds",
           "clock_state": {"before": clocks[0], "after": clocks[1]},
           "pictures": results}
    print(json.dumps(out, indent=1))
    if failed:
        sys.exit(f"mvf_unit_time: the device's outputs differ from the numpy side's: {failed}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

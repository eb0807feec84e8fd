"""GPU: `bench.py --dump-outputs DIR` at a small picture size.  Two plain runs with the same arguments must write the same arrays (the
inputs are seeded, the decode is deterministic), the plain line holds only the headline figure, and a --full run of the same
arguments decodes the same pictures in its timed region (its extra legs run before and after it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--gop", "4", "--width", "832", "--height", "480", "--steps", "3", "--warmup", "1"]


def run_bench(*extra):
    r = subprocess.run([sys.executable, "bench.py", *ARGS, *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_repeatable_and_same_as_full(tmp_path):
    lines = {name: run_bench("--dump-outputs", str(tmp_path / name), *extra)
             for name, extra in (("a", ()), ("b", ()), ("full", ("--full", "--no-verify", "--no-cpu-baseline", "--no-upload")))}
    for name in ("a", "b"):
        line = lines[name]
        assert line["steps"] == 3 and line["warmup"] == 1 and line["frames_per_step"] == 4
        assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) < 1e-6 * line["value"]
        assert not {"stages", "roofline", "verified", "cpu_baseline", "independent_frames", "incl_descriptor_upload"} & set(line), sorted(line)
    assert "stages" in lines["full"] and "roofline" in lines["full"]
    a, b, full = load(tmp_path / "a"), load(tmp_path / "b"), load(tmp_path / "full")
    assert sorted(a) == sorted(f"{c}_{k}.npy" for c in ("Y", "Cb", "Cr") for k in ("samples", "row_sums", "col_sums"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 << 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64) and a[f].shape[0] == 4, (f, a[f].dtype, a[f].shape)
        assert np.array_equal(a[f], b[f]), f"{f}: two plain runs with the same arguments differ"
        assert np.array_equal(a[f], full[f]), f"{f}: the --full run's timed region decoded something else"
    assert a["Y_row_sums.npy"].min() > 0          # decoded pictures, not untouched buffers

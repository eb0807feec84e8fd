"""CPU: bench.dump_outputs, what `bench.py --dump-outputs DIR` writes after the timed region: float arrays only, the same positions on
every call, exact row / column sums over the visible picture (not the pitch padding), and never more than bench.DUMP_BYTES in all.
The pictures here are host tensors shaped like the bench's output planes (pitched rows of 128-sample multiples)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class Picture:
    def __init__(self, rng, width, height, bd):
        self.dims = [(width, height), (width // 2, height // 2), (width // 2, height // 2)]
        dt = np.uint8 if bd == 8 else np.int16
        self.out = [torch.from_numpy(rng.integers(0, 1 << bd, size=(h, (w + 127) // 128 * 128)).astype(dt)) for (w, h) in self.dims]


def test_dump_is_float_exact_and_repeatable(tmp_path):
    rng = np.random.default_rng(3)
    pics = [Picture(rng, 200, 136, 10) for _ in range(3)]
    bench.dump_outputs(str(tmp_path / "a"), torch, pics)
    bench.dump_outputs(str(tmp_path / "b"), torch, pics)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{c}_{k}.npy" for c in ("Y", "Cb", "Cr") for k in ("samples", "row_sums", "col_sums"))
    for c, name in enumerate(("Y", "Cb", "Cr")):
        w, h = pics[0].dims[c]
        a = {k: np.load(tmp_path / "a" / f"{name}_{k}.npy") for k in ("samples", "row_sums", "col_sums")}
        for k, arr in a.items():
            assert arr.dtype in (np.float32, np.float64)
            assert np.array_equal(arr, np.load(tmp_path / "b" / f"{name}_{k}.npy"))
        visible = np.stack([p.out[c].numpy()[:, :w].astype(np.int64) for p in pics])
        assert np.array_equal(a["row_sums"], visible.sum(axis=2))
        assert np.array_equal(a["col_sums"], visible.sum(axis=1))
        # the samples: positions from the seeded generator, inside the visible picture
        g = np.random.default_rng(bench.DUMP_SEED + c)
        n = a["samples"].shape[1]
        ys, xs = g.integers(0, h, size=n), g.integers(0, w, size=n)
        assert n == min(bench.DUMP_SAMPLES[c], w * h)
        assert np.array_equal(a["samples"], visible[:, ys, xs])


def test_dump_stays_within_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 << 20)
    rng = np.random.default_rng(4)
    pics = [Picture(rng, 512, 256, 8) for _ in range(8)]
    bench.dump_outputs(str(tmp_path), torch, pics)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 3 << 20
    assert np.load(tmp_path / "Y_samples.npy").shape[0] == 8

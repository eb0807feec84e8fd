#!/usr/bin/env python3
"""Reads the geometric-partition tables out of the reference's libavcodec/vvc/vvc_data.c as data (the C-initialiser reader of
tools/ref_tables.py) and writes them to tests/golden/gpm_tables.npz, one array per table under the reference's name.  The fixture is
what tests/test_gpm_weights_cpu.py checks the library's computed masks and its small GPM tables against; no GPU test reads it.
Run where the reference tree is present; only its output is committed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_tables  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gpm_tables.npz")
TABLES = [   # (name in vvc_data.c, dtype, shape); initialisers shorter than the declared size are zero-filled, as C does
    ("ff_vvc_gpm_angle_idx", np.uint8, (64,)),
    ("ff_vvc_gpm_distance_idx", np.uint8, (64,)),
    ("ff_vvc_gpm_distance_lut", np.int8, (32,)),
    ("ff_vvc_gpm_angle_to_mirror", np.uint8, (32,)),
    ("ff_vvc_gpm_angle_to_weights_idx", np.uint8, (32,)),      # INV (-1) entries stored as 255, as in the uint8_t array
    ("ff_vvc_gpm_weights_offset_x", np.uint8, (64, 4, 4)),
    ("ff_vvc_gpm_weights_offset_y", np.uint8, (64, 4, 4)),
    ("ff_vvc_gpm_weights", np.uint8, (6, 112 * 112)),
]


def read(path=ref_tables.REF):
    text = ref_tables._strip(open(path).read()).replace("INV", "-1")
    out = {}
    for name, dt, shape in TABLES:
        vals = ref_tables._numbers(ref_tables._initialiser(text, name))
        n = int(np.prod(shape))
        assert len(vals) <= n, (name, len(vals))
        a = np.zeros(n, np.int64)
        a[:len(vals)] = vals
        out[name] = (a & 0xFF).astype(np.uint8).view(dt).reshape(shape) if dt == np.int8 else a.astype(dt).reshape(shape)
    return out


def main():
    t = read()
    np.savez_compressed(OUT, **t)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

"""Loader of the reference shim (oracle/_ref/libvvcref.so, built by `make -C oracle ref`) for the tests that pin the oracle.

The library exists only where the reference tree was present at build time; it is never committed.  `REFERENCE` names the
tree the recipe builds from (the default of oracle/Makefile unless the environment overrides it).  Plain module: tools/gen_golden.py
uses it too; what needs pytest is in tests/golden_check.py."""
import ctypes
import json
import os
import subprocess
import sys

import ref_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libvvcref.so")
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "ref_slots.json")


def reference_tree():
    """Path of the reference tree the recipe would build from, or None when it is not on this machine (oracle/Makefile decides)."""
    out = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref-tree"], capture_output=True, text=True, check=True).stdout.strip()
    return out or None


_made = False


def load():
    """The bound reference library, or None when it has not been built.  The first call brings it up to date with its sources
    (`make ref`, as conftest.load_oracle does for the oracle: a no-op when nothing changed and where there is no reference tree), so
    that a library left behind by a build of another revision is not mistaken for this one's."""
    global _made
    if not _made:
        _made = True
        done = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], capture_output=True, text=True)
        if done.returncode:          # a shim that no longer compiles: say why, the tests then report the library as missing or stale
            print(f"`make -C oracle ref` failed ({done.returncode}):\n{done.stdout[-2000:]}{done.stderr[-4000:]}", file=sys.stderr)
    if not os.path.exists(LIB_PATH):
        return None
    return ref_cases.bind(ctypes.CDLL(LIB_PATH), "ref_")


def load_oracle():
    import conftest
    return ref_cases.bind(conftest.load_oracle(), "orc_")


def load_golden():
    """slots[slot][group] = [input digest, output digest] of tests/golden/ref_slots.json."""
    with open(GOLDEN_PATH) as f:
        return json.load(f)["slots"]

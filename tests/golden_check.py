"""Shared body of tests/test_golden_cpu.py and tests/test_golden_gpu.py: run a slot's groups against tests/golden/ref_slots.json."""
import hashlib

import pytest

import ref_cases
import ref_ctx_cases


def check_slot(golden, slot, fn, bd=None, explain=None):
    """Run the slot's groups (of bit depth `bd`, or all) through `fn` against the digests; returns the number of groups checked."""
    rec, n = golden[slot], 0
    for gid, cases in ref_cases.groups(slot):
        if bd is not None and cases[0].key[0] != bd:
            continue
        key = gid.split("/", 1)[1]
        assert key in rec, f"group {gid} is not in ref_slots.json: regenerate it (tests/golden/README.md)"
        h_in = hashlib.sha256()
        for c in cases:
            ref_cases.input_digest(h_in, c)
        assert h_in.hexdigest() == rec[key][0], f"generator drifted: the inputs of group {gid} no longer hash to the recorded digest"
        h_out, outs = hashlib.sha256(), []
        for c in cases:
            outs.append(ref_cases.outputs(c, *ref_cases.run(c, fn)))
            ref_cases.output_digest(h_out, outs[-1])
        if h_out.hexdigest() != rec[key][1]:
            detail = explain(cases, outs) if explain else "; ".join(str(c.params) for c in cases[:4]) + " ..."
            pytest.fail(f"group {gid}: outputs do not hash to the reference's digest: {detail}")
        n += 1
    return n


def check_ctx_slot(golden, slot, side, bd=None, explain=None):
    """The same for a slot that takes the decoder's context (tests/ref_ctx_cases.py), run by `side`."""
    rec, n = golden[slot], 0
    for gid, cases in ref_ctx_cases.groups(slot):
        if bd is not None and cases[0].key[0] != bd:
            continue
        key = gid.split("/", 1)[1]
        assert key in rec, f"group {gid} is not in ref_slots.json: regenerate it (tests/golden/README.md)"
        h_in = hashlib.sha256()
        ref_ctx_cases.group_input_digest(h_in, cases)
        assert h_in.hexdigest() == rec[key][0], f"generator drifted: the inputs of group {gid} no longer hash to the recorded digest"
        h_out, outs = hashlib.sha256(), []
        for c in cases:
            outs.append(ref_ctx_cases.run(c, side))
            ref_cases.output_digest(h_out, outs[-1])
        if h_out.hexdigest() != rec[key][1]:
            detail = explain(cases, outs) if explain else "; ".join(str(c.params) for c in cases[:4]) + " ..."
            pytest.fail(f"group {gid}: outputs do not hash to the reference's digest: {detail}")
        n += 1
    return n

#!/usr/bin/env python3
"""Regenerate tests/golden/ref_slots.json, tests/golden/ref_passes.json, tests/golden/ref_inter.json, tests/golden/ref_recon.json,
tests/golden/ref_picture.json, tests/golden/ref_decoded.json and tests/golden/ref_extremes.json (the full-scale pictures of tests/extreme_cases.py, in the format of ref_passes.json / ref_inter.json): SHA-256
digests of what the reference's own C path computes on the case lists of tests/ref_cases.py, of what its in-loop filter callers compute on
the pictures of tests/ref_pass_cases.py, of what its inter prediction callers compute on the pictures of tests/ref_inter_cases.py, and of what
ff_vvc_reconstruct computes on the pictures of tests/ref_recon_cases.py.

Needs oracle/_ref/libvvcref.so (`make -C oracle ref`, or __graft_entry__.build() where the reference tree is present).
For every group of at most 64 cases (slot, bit depth, table indices) the file holds [digest of the concatenated inputs,
digest of the concatenated outputs]; it holds no samples.  A regeneration may only add slots and groups: a recorded digest that
would change is an error (the case generator drifted, or the reference did), unless --replace says that the change is meant.
ref_passes.json holds per picture one digest of the inputs, one per output table and one per plane after each stage, under the same rule.
ref_inter.json holds per picture one digest of the inputs and one per output plane; regular pictures add tab_dmvr_mvf, CIIP pictures the
scratch, the intra weights and the patched .joint bytes; same rule.  Its digests are layout-independent: planes cropped to their width,
MvField entries with the pad bytes zeroed.
ref_recon.json holds per picture one digest of the inputs, one per plane after ff_vvc_reconstruct and one of the chroma scales the reference
cached for the 64x64 units whose blocks the host routes to the TB passes; same rule.
ref_picture.json holds per picture of tests/ref_picture_cases.py one digest of the inputs, one per plane after ff_vvc_reconstruct, one per plane
after ff_vvc_lmcs_filter, tab_dmvr_mvf and the routed units' chroma scales, all from ref_decode_picture; same rule, layout-independent.
ref_recon_extremes.json holds the same record as ref_recon.json per directed worst-case picture of tests/recon_extreme_cases.py; same rule.
ref_decoded.json holds per picture of tests/ref_decoded_cases.py one digest of the inputs, tab_dmvr_mvf, the ten bS / filter-length tables and
the QP tables the reference's deblocking read, and one per plane after the horizontal pass, SAO and ALF, from ref_decode_picture followed by
ref_deblock_picture, ref_sao_picture and ref_alf_picture on its output; same rule.
Usage: python tools/gen_golden.py [--check | --replace]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_cases  # noqa: E402
import ref_lib    # noqa: E402

try:                  # the tool is also imported by the tests of revisions whose tests/ has no context slots yet
    import ref_ctx_cases  # noqa: E402
except ImportError:
    ref_ctx_cases = None

try:                  # ... or no whole-picture passes yet (ref_passes.json is then left alone)
    import ref_pass_cases  # noqa: E402
except ImportError:
    ref_pass_cases = None

try:                  # ... or no inter prediction pictures yet (ref_inter.json is then left alone)
    import ref_inter_cases  # noqa: E402
except ImportError:
    ref_inter_cases = None

try:                  # ... or no RECON pictures yet (ref_recon.json is then left alone)
    import ref_recon_cases  # noqa: E402
except ImportError:
    ref_recon_cases = None

try:                  # ... or no whole-picture pin of prediction + reconstruction + inverse LMCS yet (ref_picture.json is then left alone)
    import ref_picture_cases  # noqa: E402
except ImportError:
    ref_picture_cases = None

try:                  # ... or no full-scale pictures yet (ref_extremes.json is then left alone)
    import extreme_cases  # noqa: E402
except ImportError:
    extreme_cases = None

try:                  # ... or no whole decoded pictures yet (ref_decoded.json is then left alone)
    import ref_decoded_cases  # noqa: E402
except ImportError:
    ref_decoded_cases = None

try:                  # ... or no worst-case RECON pictures yet (ref_recon_extremes.json is then left alone)
    import recon_extreme_cases  # noqa: E402
except ImportError:
    recon_extreme_cases = None

CONTEXT_SLOTS_AFTER = "ilfnst_transform"          # the context slots follow vvc_intra.c's static functions in the file


def slot_order():
    """[(case module, slot)] in the order of the file.  The last slot stays the last: a slot added anywhere before it shows in
    `git diff` of the file as added lines only."""
    order = [(ref_cases, slot) for slot in ref_cases.SLOTS]
    if ref_ctx_cases is not None:
        at = [slot for _, slot in order].index(CONTEXT_SLOTS_AFTER) + 1
        order[at:at] = [(ref_ctx_cases, slot) for slot in ref_ctx_cases.SLOTS]
    return order

PATH = ref_lib.GOLDEN_PATH


def group_digests(cases, fn):
    """(input digest, output digest) of one group run through `fn`."""
    h_in, h_out = hashlib.sha256(), hashlib.sha256()
    for c in cases:
        ref_cases.input_digest(h_in, c)
        ref_cases.output_digest(h_out, ref_cases.outputs(c, *ref_cases.run(c, fn)))
    return h_in.hexdigest(), h_out.hexdigest()


def ctx_group_digests(cases, side):
    """The same for a group of context cases (tests/ref_ctx_cases.py) run by `side`."""
    h_in, h_out = hashlib.sha256(), hashlib.sha256()
    ref_ctx_cases.group_input_digest(h_in, cases)
    for c in cases:
        ref_cases.output_digest(h_out, ref_ctx_cases.run(c, side))
    return h_in.hexdigest(), h_out.hexdigest()


def generate(lib, prefix):
    doc = {"source": "reference C path (ff_vvc_dsp_init slots and vvc_intra.c / vvc_itx_1d.c helpers) through oracle/ref_shim.c on tests/ref_cases.py",
           "format": "slots[slot][group] = [sha256 of inputs, sha256 of outputs]; group = bit depth and table indices / chunk of 64 cases",
           "slots": {}}
    side = None
    for module, slot in slot_order():
        if module is ref_cases:
            fn = getattr(lib, prefix + slot)
            doc["slots"][slot] = {gid.split("/", 1)[1]: list(group_digests(cases, fn)) for gid, cases in ref_cases.groups(slot)}
        else:
            side = side or module.reference_side(lib)
            doc["slots"][slot] = {gid.split("/", 1)[1]: list(ctx_group_digests(cases, side)) for gid, cases in module.groups(slot)}
    return doc


def dumps(doc):
    lines = ["{", f' "source": {json.dumps(doc["source"])},', f' "format": {json.dumps(doc["format"])},', ' "slots": {']
    slots = list(doc["slots"].items())
    for i, (slot, grp) in enumerate(slots):
        lines.append(f"  {json.dumps(slot)}: {{")
        items = list(grp.items())
        lines += [f"   {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" + ("," if j + 1 < len(items) else "") for j, (k, v) in enumerate(items)]
        lines.append("  }" + ("," if i + 1 < len(slots) else ""))
    lines += [" }", "}", ""]
    return "\n".join(lines)


def generate_passes(lib, orc):
    """The document of ref_passes.json: the reference's whole-picture runs (oracle/ref_shim_filter.c).  `orc` only builds the pictures that
    bs_rec_cases caches together with the oracle's tables; nothing of the oracle's enters the file."""
    return {"source": "reference in-loop filter callers (ff_vvc_deblock_vertical / _horizontal, ff_vvc_sao_filter, ff_vvc_alf_filter) through "
                      "oracle/ref_shim_filter.c on tests/ref_pass_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the ten bS / filter-length tables; the planes after each stage (v, h, sao, alf + component)",
            "pictures": {name: ref_pass_cases.host_digests(orc, lib, "ref", name) for name in ref_pass_cases.picture_names()}}


def dumps_passes(doc):
    lines = ["{", f' "source": {json.dumps(doc["source"])},', f' "format": {json.dumps(doc["format"])},', ' "pictures": {']
    pics = list(doc["pictures"].items())
    for i, (name, rec) in enumerate(pics):
        lines.append(f"  {json.dumps(name)}: {{")
        items = list(rec.items())
        lines += [f"   {json.dumps(k)}: {json.dumps(v)}" + ("," if j + 1 < len(items) else "") for j, (k, v) in enumerate(items)]
        lines.append("  }" + ("," if i + 1 < len(pics) else ""))
    lines += [" }", "}", ""]
    return "\n".join(lines)


def generate_inter(lib):
    """The document of ref_inter.json: the reference's whole-picture inter prediction runs (oracle/ref_shim_inter.c); nothing of the oracle's
    enters the file."""
    return {"source": "reference inter prediction callers (ff_vvc_predict_inter, ff_vvc_predict_ciip) through oracle/ref_shim_inter.c on "
                      "tests/ref_inter_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the planes after prediction (p + component); dmvr = tab_dmvr_mvf, pad bytes zeroed; "
                      "CIIP: scratch, weights (int32 [unit][3]), joint (the command array's .joint bytes after the patch)",
            "pictures": {name: ref_inter_cases.host_digests(lib, "ref", name) for name in ref_inter_cases.picture_names()}}


def generate_recon(lib):
    """The document of ref_recon.json: the reference's RECON walk over whole pictures (ref_recon_picture of oracle/ref_shim_intra.c); nothing
    of the oracle's enters the file."""
    return {"source": "reference RECON stage (ff_vvc_reconstruct per CTU) through oracle/ref_shim_intra.c on tests/ref_recon_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the planes after reconstruction (p + component); scale = (unit x, unit y, chroma scale) of "
                      "the 64x64 units whose blocks go to the TB passes, as the reference cached them",
            "pictures": {name: ref_recon_cases.reference_digests(lib, name) for name in ref_recon_cases.picture_names()}}


def generate_recon_extremes(lib):
    """The document of ref_recon_extremes.json: the reference's RECON walk over the directed worst-case pictures; nothing of the oracle's
    enters the file."""
    return {"source": "reference RECON stage (ff_vvc_reconstruct per CTU) through oracle/ref_shim_intra.c on tests/recon_extreme_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the planes after reconstruction (p + component); scale = (unit x, unit y, chroma scale) of "
                      "the 64x64 units whose blocks go to the TB passes, as the reference cached them",
            "pictures": {name: recon_extreme_cases.reference_digests(lib, name) for name in recon_extreme_cases.picture_names()}}


def generate_extremes(lib):
    """The document of ref_extremes.json: the reference's whole-picture runs on the full-scale pictures of tests/extreme_cases.py; nothing of
    the oracle's enters the file."""
    return {"source": "reference in-loop filter and inter prediction callers through oracle/ref_shim_filter.c and oracle/ref_shim_inter.c on "
                      "tests/extreme_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the planes after the stage (sao / alf / p + component); regular inter pictures add "
                      "dmvr = tab_dmvr_mvf, pad bytes zeroed; CIIP: scratch, weights, joint as in ref_inter.json",
            "pictures": {name: extreme_cases.host_digests(lib, "ref", name) for name in extreme_cases.picture_names()}}


def generate_picture(lib):
    """The document of ref_picture.json: the reference's three calls per CTU over whole pictures (ref_decode_picture of
    oracle/ref_shim_picture.c); nothing of the oracle's enters the file."""
    return {"source": "reference picture chain (ff_vvc_predict_inter, ff_vvc_reconstruct with ff_vvc_predict_ciip, ff_vvc_lmcs_filter per CTU) through "
                      "oracle/ref_shim_picture.c on tests/ref_picture_cases.py",
            "format": "pictures[name][key] = sha256: inputs; the planes after reconstruction (r + component) and after inverse LMCS (p + component); "
                      "dmvr = tab_dmvr_mvf, pad bytes zeroed; scale = (unit x, unit y, chroma scale) of the 64x64 units whose blocks go to the TB passes",
            "pictures": {name: ref_picture_cases.reference_digests(lib, name) for name in ref_picture_cases.picture_names()}}


def generate_decoded(lib, orc):
    """The document of ref_decoded.json: the reference's picture chain followed by its three in-loop filter callers.  `orc` draws what the
    description leaves to the reconstructed luma (the LADF bounds, from a plane ref_picture.json pins to the reference's); nothing the
    oracle computed enters the file."""
    return {"source": "reference picture chain (ref_decode_picture of oracle/ref_shim_picture.c) followed by ff_vvc_deblock_vertical / _horizontal, "
                      "ff_vvc_sao_filter and ff_vvc_alf_filter (oracle/ref_shim_filter.c) on tests/ref_decoded_cases.py",
            "format": "pictures[name][key] = sha256: inputs; dmvr = tab_dmvr_mvf, pad bytes zeroed; the ten bS / filter-length tables; the QP tables "
                      "painted from the units; the planes after the horizontal pass, SAO and ALF (h, sao, alf + component)",
            "pictures": {name: ref_decoded_cases.reference_digests(lib, orc, name) for name in ref_decoded_cases.picture_names()}}


def changed_digests(old, new):
    """Groups of `old` that `new` drops or records differently: [] when `new` only adds to `old`."""
    return [f"{slot}/{key}" for slot, grp in old.items() for key, rec in grp.items() if new.get(slot, {}).get(key) != rec]


def main():
    lib = ref_lib.load()
    if lib is None:
        sys.exit(f"{ref_lib.LIB_PATH} is missing: run `make -C oracle ref` where the reference tree is present")
    text = dumps(generate(lib, "ref_"))
    passes = dumps_passes(generate_passes(lib, ref_lib.load_oracle()))
    p_path = ref_pass_cases.GOLDEN_PATH
    inter = dumps_passes(generate_inter(lib)) if ref_inter_cases is not None else None
    i_path = ref_inter_cases.GOLDEN_PATH if ref_inter_cases is not None else None
    recon = dumps_passes(generate_recon(lib)) if ref_recon_cases is not None else None
    r_path = ref_recon_cases.GOLDEN_PATH if ref_recon_cases is not None else None
    extremes = dumps_passes(generate_extremes(lib)) if extreme_cases is not None else None
    x_path = extreme_cases.GOLDEN_PATH if extreme_cases is not None else None
    whole = dumps_passes(generate_picture(lib)) if ref_picture_cases is not None else None
    w_path = ref_picture_cases.GOLDEN_PATH if ref_picture_cases is not None else None
    decoded = dumps_passes(generate_decoded(lib, ref_lib.load_oracle())) if ref_decoded_cases is not None else None
    d_path = ref_decoded_cases.GOLDEN_PATH if ref_decoded_cases is not None else None
    rx = dumps_passes(generate_recon_extremes(lib)) if recon_extreme_cases is not None else None
    rx_path = recon_extreme_cases.GOLDEN_PATH if recon_extreme_cases is not None else None
    if "--check" in sys.argv:
        for path, want in ((PATH, text), (p_path, passes), (i_path, inter), (r_path, recon), (x_path, extremes), (w_path, whole), (d_path, decoded),
                           (rx_path, rx)):
            if path is None:
                continue
            if not os.path.exists(path):
                sys.exit(f"{os.path.relpath(path, ROOT)} is missing")
            with open(path) as f:
                if f.read() != want:
                    sys.exit(f"{os.path.relpath(path, ROOT)} is stale")
        sys.exit(0)
    if "--replace" not in sys.argv:
        bad = changed_digests(ref_lib.load_golden(), json.loads(text)["slots"]) if os.path.exists(PATH) else []
        bad += changed_digests(ref_pass_cases.load_golden(), json.loads(passes)["pictures"]) if os.path.exists(p_path) else []
        if i_path and os.path.exists(i_path):
            bad += changed_digests(ref_inter_cases.load_golden(), json.loads(inter)["pictures"])
        if r_path and os.path.exists(r_path):
            bad += changed_digests(ref_recon_cases.load_golden(), json.loads(recon)["pictures"])
        if x_path and os.path.exists(x_path):
            bad += changed_digests(extreme_cases.load_golden(), json.loads(extremes)["pictures"])
        if w_path and os.path.exists(w_path):
            bad += changed_digests(ref_picture_cases.load_golden(), json.loads(whole)["pictures"])
        if d_path and os.path.exists(d_path):
            bad += changed_digests(ref_decoded_cases.load_golden(), json.loads(decoded)["pictures"])
        if rx_path and os.path.exists(rx_path):
            bad += changed_digests(recon_extreme_cases.load_golden(), json.loads(rx)["pictures"])
        if bad:
            sys.exit(f"{len(bad)} recorded groups would change or vanish (first: {bad[:4]}): nothing written; --replace if that is meant")
    with open(PATH, "w") as f:
        f.write(text)
    n = sum(len(g) for g in json.loads(text)["slots"].values())
    print(f"wrote {PATH}: {n} groups, {len(text)} bytes")
    with open(p_path, "w") as f:
        f.write(passes)
    print(f"wrote {p_path}: {len(json.loads(passes)['pictures'])} pictures, {len(passes)} bytes")
    if i_path:
        with open(i_path, "w") as f:
            f.write(inter)
        print(f"wrote {i_path}: {len(json.loads(inter)['pictures'])} pictures, {len(inter)} bytes")
    if r_path:
        with open(r_path, "w") as f:
            f.write(recon)
        print(f"wrote {r_path}: {len(json.loads(recon)['pictures'])} pictures, {len(recon)} bytes")
    if x_path:
        with open(x_path, "w") as f:
            f.write(extremes)
        print(f"wrote {x_path}: {len(json.loads(extremes)['pictures'])} pictures, {len(extremes)} bytes")
    if w_path:
        with open(w_path, "w") as f:
            f.write(whole)
        print(f"wrote {w_path}: {len(json.loads(whole)['pictures'])} pictures, {len(whole)} bytes")
    if d_path:
        with open(d_path, "w") as f:
            f.write(decoded)
        print(f"wrote {d_path}: {len(json.loads(decoded)['pictures'])} pictures, {len(decoded)} bytes")

    if rx_path:
        with open(rx_path, "w") as f:
            f.write(rx)
        print(f"wrote {rx_path}: {len(json.loads(rx)['pictures'])} pictures, {len(rx)} bytes")


if __name__ == "__main__":
    main()

"""CPU: the oracle against the reference decoder's own C path, bit-exactly, slot by slot.

`ref` is oracle/_ref/libvvcref.so (oracle/ref_shim.c linked against the reference's static libraries by `make -C oracle ref`).
Every slot runs its committed case list (tests/ref_cases.py, seed 0) and a wider sweep: rounds of freshly drawn cases (seeds 1, 2, ...)
until at least SWEEP of them are compared.  The helpers of ref_cases.EXHAUSTIVE list their whole domain and have no sweep.
Where the library is absent the comparisons skip; where the reference tree is present and the library is not (the loader's `make ref`
failed: its messages are on stderr), one test fails.
Run with -rA (or -s) to see how many cases each slot compared."""
import ctypes

import numpy as np
import pytest

import ctx_mirror as cm
import ref_cases
import ref_ctx_cases as rcc
import ref_lib
from ffvvc_amd import abi

SWEEP = 2000          # fresh cases per slot in the sweep, at the least (whole rounds)


@pytest.fixture(scope="module")
def ref():
    lib = ref_lib.load()
    if lib is None:
        pytest.skip("oracle/_ref/libvvcref.so is not built (no reference tree on this machine)")
    return lib


@pytest.fixture(scope="module")
def orc():
    return ref_lib.load_oracle()


def test_reference_library_is_built_where_the_tree_is():
    tree = ref_lib.reference_tree()
    if tree is None:
        pytest.skip("no reference tree on this machine")
    assert ref_lib.load() is not None, f"the reference tree is at {tree} but {ref_lib.LIB_PATH} is missing: `make -C oracle ref` fails (see stderr)"


def compare(orc, ref, slot, seed):
    f_orc, f_ref = getattr(orc, "orc_" + slot), getattr(ref, "ref_" + slot)
    lst = ref_cases.cases(slot, seed)
    if lst[0].ret and not any(isinstance(a, ref_cases.Buf) for c in lst[:64] for a in c.args):          # integers in, one integer out
        for c in lst:
            want, got = f_ref(*c.args), f_orc(*c.args)
            assert want == got, f"oracle differs from the reference (seed {seed}): {slot} {c.params}: want {want} got {got}"
        return len(lst)
    for c in lst:
        want = ref_cases.outputs(c, *ref_cases.run(c, f_ref))
        got = ref_cases.outputs(c, *ref_cases.run(c, f_orc))
        diff = ref_cases.first_difference(c, want, got)
        assert diff is None, f"oracle differs from the reference (seed {seed}): {diff}"
    return len(lst)


@pytest.mark.parametrize("slot", ref_cases.SLOTS)
def test_case_list(orc, ref, slot):
    n = compare(orc, ref, slot, 0)
    assert n > 0
    print(f"{slot}: {n} listed cases compared, bit-exact")


@pytest.mark.parametrize("slot", [s for s in ref_cases.SLOTS if s not in ref_cases.EXHAUSTIVE])
def test_sweep(orc, ref, slot):
    n, seed = 0, 0
    while n < SWEEP:
        seed += 1
        k = compare(orc, ref, slot, seed)
        assert k > 0
        n += k
    assert n >= SWEEP
    print(f"{slot}: {n} sweep cases compared in {seed} rounds, bit-exact")


@pytest.mark.parametrize("slot", ["fetch_samples", "avg", "lmcs_filter", "lf_ladf_level", "alf_recon_coeff_and_clip", "intra_wide_angle", "dequant", "ilfnst_transform"])
def test_sweep_rounds_are_fresh(slot):
    """No case of a sweep round has the inputs of a case of the list or of an earlier round, the fixed patterns (all-minimum, all-maximum,
    checkerboard) included.  Checked on the slots with the shortest lists, which need the most rounds; the argument-only helper may
    draw a tuple twice, so there the rounds are only required to differ from each other as a whole."""
    import hashlib
    seen, rounds = set(), set()
    for seed in range(4):
        whole = hashlib.sha256()
        for c in ref_cases.cases(slot, seed):
            h = hashlib.sha256()
            ref_cases.input_digest(h, c)
            ref_cases.input_digest(whole, c)
            if slot != "intra_wide_angle":
                assert h.digest() not in seen, f"seed {seed} repeats a case: {c.params}"
            seen.add(h.digest())
        assert whole.digest() not in rounds, f"round {seed} repeats an earlier round"
        rounds.add(whole.digest())


def test_case_module_restatements(ref):
    """The two small restatements the case module itself uses to stay inside the domain agree with the reference."""
    for (w, h) in ref_cases.INTRA_SIZES:
        if max(w, h) > 16 * min(w, h):
            continue
        for m in range(2, 67):
            mode = ref_cases.wide_angle(m, w, h)
            assert mode == ref.ref_intra_wide_angle(0, 0, w, h, w, h, m)
            if mode not in (18, 50):
                assert int(ref_cases.need_pdpc(w, h, mode)) == ref.ref_intra_need_pdpc(w, h, 0, mode, 0), (w, h, mode)


def test_ilfnst_cases_take_every_route_to_the_mode(ref):
    """ref_ilfnst_transform hands the reference the mode by one of the routes derive_ilfnst_pred_mode_intra has, chosen from the
    arguments: over the committed list every one of them must be taken, and every call must come out with the mode it was given."""
    ref.ref_ilfnst_route_calls.argtypes, ref.ref_ilfnst_route_calls.restype = [ctypes.c_int], ctypes.c_int
    ref.ref_ilfnst_route_calls(-1)
    lst = ref_cases.cases("ilfnst_transform")
    for c in lst:
        ref_cases.run(c, ref.ref_ilfnst_transform)
    names = ["luma mode", "luma MIP -> planar", "CCLM -> collocated luma mode (ipm)", "CCLM -> collocated MIP (imf) -> planar",
             "CCLM -> collocated IBC (cpm) -> DC", "CCLM -> collocated palette (cpm) -> DC", "chroma mode"]
    calls = {n: ref.ref_ilfnst_route_calls(i) for i, n in enumerate(names)}
    assert ref.ref_ilfnst_route_calls(len(names)) == -1
    assert all(calls.values()) and sum(calls.values()) == len(lst), calls
    print(calls)


# ------------------------------------------------------------------------------------------------ the slots that take the decoder's context
#
# Both sides start from the same mirror context (tests/ref_ctx_cases.py): the reference runs its real slot on real structs, the project
# flattens the context with the host shim (vvc355_ctx_flatten_*) and runs the oracle's flat form: the flattening and the oracle are pinned
# together.



@pytest.fixture(scope="module")
def project_side(orc):
    return rcc.oracle_side(orc, cm.load_host())


@pytest.fixture(scope="module")
def reference_side(ref):
    return rcc.reference_side(ref)


def compare_ctx(reference_side, project_side, slot, seed):
    lst = rcc.cases(slot, seed)
    changed = 0
    for c in lst:
        want, got = rcc.run(c, reference_side), rcc.run(c, project_side)
        diff = rcc.first_difference(c, want, got)
        assert diff is None, f"the host shim + oracle differ from the reference (seed {seed}): {diff}"
        changed += c.ret or any(not np.array_equal(a, b) for a, b in zip(want, c.pic.planes)) or (c.coeff is not None and not np.any(want[3] == 0x5A5A5A))
    assert changed > 0.9 * len(lst), "most calls must write something"
    return len(lst)


@pytest.mark.parametrize("slot", rcc.SLOTS)
def test_context_case_list(reference_side, project_side, slot):
    n = compare_ctx(reference_side, project_side, slot, 0)
    assert n > 0
    print(f"{slot}: {n} listed cases compared, bit-exact")


@pytest.mark.parametrize("slot", rcc.SLOTS)
def test_context_sweep(reference_side, project_side, slot):
    n, seed = 0, 0
    while n < SWEEP:
        seed += 1
        k = compare_ctx(reference_side, project_side, slot, seed)
        assert k > 0
        n += k
    print(f"{slot}: {n} sweep cases compared in {seed} rounds, bit-exact")


def test_mirror_layouts_agree(ref):
    """The reference shim declares the layout of include/vvc_mi355_ctx.h under names of its own; the ctypes mirror is the third copy."""
    L, F, C = cm.VVCLocalContext, cm.VVCFrameContext, cm.CodingUnit
    want = [ctypes.sizeof(L), ctypes.sizeof(F), ctypes.sizeof(C), L.num_ras.offset, L.end_of_tiles_x.offset, L.lmcs.offset, F.imf.offset, F.lmcs.offset,
            C.bdpcm_flag.offset]
    ref.ref_ctx_layout.argtypes, ref.ref_ctx_layout.restype = [ctypes.c_int], ctypes.c_int
    assert [ref.ref_ctx_layout(i) for i in range(len(want))] == want


def test_lmcs_scale_with_a_matching_cache(reference_side, project_side):
    """The reference keeps the scale of the last 64x64 unit in lc->lmcs; the project derives it on every call.  The cold call must leave
    this unit's position and the scale the oracle derives in the cache, and a second call that finds them there must still agree."""
    n = 0
    for c in rcc.cases("lmcs_scale_chroma")[::3]:
        rcc.run(c, reference_side)
        got = rcc.run(c, project_side)
        size = min(c.params["ctb"], 64)
        assert reference_side.cache == (c.args[2] & ~(size - 1), c.args[3] & ~(size - 1), project_side.scale), c.params
        warm = rcc.with_cache(c, reference_side.cache[2])
        diff = rcc.first_difference(warm, rcc.run(warm, reference_side), got)
        assert diff is None, diff
        n += 1
    assert n > 100
    print(f"lmcs_scale_chroma: {n} cases repeated with a matching cache")


def test_recon_walk_availability_matches_the_reference(orc, ref, reference_side):
    """The oracle's own RECON walk (orc_recon_debug_job) derives the availability of every block from the command lists; the
    reference answers the same question on the mirror context of the same block."""
    orc.orc_recon_debug_job.argtypes = [ctypes.POINTER(abi.ReconFrame), ctypes.c_int, ctypes.c_int, ctypes.POINTER(abi.IntraJob)]
    orc.orc_recon_debug_job.restype = None
    frames, n = {}, 0
    for c in rcc.cases("intra_pred")[::4]:
        pic = c.pic
        if pic.idx not in frames:
            work = pic.work
            cmds = work.bind(0)
            frames[pic.idx] = (cmds, work.frame([0, 0, 0], [pic.w, pic.w >> pic.hs, pic.w >> pic.hs], cmds.ctypes.data, work.ctus.ctypes.data, work.order.ctypes.data, 0,
                                                work.slice_idx.ctypes.data, work.col_bd.ctypes.data, work.row_bd.ctypes.data, wpp=pic.wpp))
        job = abi.IntraJob()
        orc.orc_recon_debug_job(ctypes.byref(frames[pic.idx][1]), c.params["rs"], c.params["cmd"], ctypes.byref(job))
        x0, y0, _, _, c_idx = c.args
        lc, keep = rcc.context(c, pic.planes)
        at = (x0 >> (pic.hs if c_idx else 0), y0 >> (pic.vs if c_idx else 0), rcc.UNBOUNDED, c_idx)
        assert (job.top_avail, job.left_avail) == (ref.ref_top_available(lc, *at), ref.ref_left_available(lc, *at)), c.params
        assert job.cand_up_left == c.cand_up_left, c.params
        n += 1
    assert n > 200
    print(f"{n} blocks: the RECON walk's availability equals the reference's")


def test_context_cases_visit_what_they_must(orc):
    """The committed lists reach the situations the pin is for (counted on the jobs the host shim derives; needs no reference)."""
    host = cm.load_host()
    rcc.oracle_side(orc, host)          # binds the flatten entries
    seen = {}

    def hit(name):
        seen[name] = seen.get(name, 0) + 1

    pre_modes, mapped = set(), set()
    for c in rcc.cases("intra_pred"):
        pic, (x0, y0, bw, bh, c_idx) = c.pic, c.args
        lc, keep = rcc.context(c, pic.planes)
        j = abi.IntraJob()
        host.vvc355_ctx_flatten_intra_pred(lc, x0, y0, bw, bh, c_idx, ctypes.byref(j))
        ctb_c = (1 << pic.ctb_log2) >> (pic.vs if c_idx else 0)
        hs = pic.hs if c_idx else 0
        hit(f"bd{pic.bd}"), hit(f"size{max(j.w, j.h)}"), hit(f"size{min(j.w, j.h)}")
        if not j.top_avail and not j.left_avail and not j.cand_up_left:
            hit("nothing available")
        if j.w < j.top_avail < j.w + j.h:
            hit("top-right partly available")
        if j.h < j.left_avail < j.h + j.w:
            hit("bottom-left partly available")
        if j.y % ctb_c == 0 and c.ctu[1] and c.ctu[2] < pic.w and (c.ctu[2] >> hs) - j.x < j.w + j.h and not pic.wpp:
            hit("tile end clips the top row")          # an interior tile boundary, and no wavefront that would clip there as well
        if j.y % ctb_c == 0 and c.ctu[1] and pic.wpp and j.top_avail < j.w + j.h and (c.ctu[2] >> hs) - j.x >= j.w + j.h:
            hit("wavefront clips the top row")
        if not c_idx:
            hit(f"reference line {j.ref_idx}")
            if j.isp_split:
                hit("ISP")
                if j.w == 4 and j.cb_width in (4, 8) and j.cb_height == j.h:
                    hit(f"ISP vertical parts {j.cb_width // 4} wide")
            if j.is_mip:
                hit("MIP")
            if j.bdpcm_flag:
                hit("BDPCM luma")
            if j.w != j.h and not j.is_mip and c.cu["intra_pred_mode_y"] >= 2:
                pre_modes.add(c.cu["intra_pred_mode_y"]), mapped.add(j.mode)
        else:
            if j.bdpcm_flag:
                hit("BDPCM chroma")
            if j.is_mip:
                hit("MIP chroma direct")
            if c.mip[0] and not j.is_mip:
                hit("MIP luma, chroma not direct")
        del keep
    for name in ["bd8", "bd10", "bd12", "size4", "size8", "size16", "size32", "size64", "nothing available", "top-right partly available",
                 "bottom-left partly available", "tile end clips the top row", "wavefront clips the top row", "reference line 0", "reference line 1",
                 "reference line 2", "ISP", "ISP vertical parts 1 wide", "ISP vertical parts 2 wide", "MIP", "BDPCM luma", "BDPCM chroma", "MIP chroma direct",
                 "MIP luma, chroma not direct"]:
        assert seen.get(name), f"intra_pred: no case with: {name} (have {seen})"
    assert seen["tile end clips the top row"] >= 4, seen
    assert pre_modes == set(range(2, 67)), sorted(set(range(2, 67)) - pre_modes)
    every = set(range(-14, 81)) - {0, 1}          # after the mapping: 2 .. 66 and both wide-angle ranges whole
    assert mapped >= every, f"angular modes that meet no non-square block: {sorted(every - mapped)}"

    cclm = {}
    for c in rcc.cases("intra_cclm_pred"):
        pic, (x0, y0, bw, bh) = c.pic, c.args
        for name in (f"mode{c.cu['intra_pred_mode_c']}", f"collocated{pic.collocated}" if pic.vs else None, f"chroma{pic.hs}{pic.vs}",
                     "CTU boundary row" if y0 % (1 << pic.ctb_log2) == 0 and c.ctu[1] else None, "left picture edge" if x0 == 0 else None,
                     "top picture edge" if y0 == 0 else None):
            if name:
                cclm[name] = cclm.get(name, 0) + 1
    for name in ["mode81", "mode82", "mode83", "collocated0", "collocated1", "chroma11", "chroma10", "chroma00", "CTU boundary row", "left picture edge", "top picture edge"]:
        assert cclm.get(name), f"intra_cclm_pred: no case with: {name} (have {cclm})"

    lmcs = {}
    for c in rcc.cases("lmcs_scale_chroma"):
        pic = c.pic
        lc, keep = rcc.context(c, pic.planes)
        j = abi.LmcsScaleJob()
        host.vvc355_ctx_flatten_lmcs_scale(lc, c.args[2], c.args[3], ctypes.byref(j))
        cut = j.x_vpdu + j.size_y > pic.w or j.y_vpdu + j.size_y > pic.h
        for name in (f"{j.avail_t + j.avail_l} neighbours", "unit cut by the picture edge" if cut else None, "narrow bins" if pic.bins != (0, 15) else "full bins"):
            if name:
                lmcs[name] = lmcs.get(name, 0) + 1
        del keep
    for name in ["0 neighbours", "1 neighbours", "2 neighbours", "unit cut by the picture edge", "narrow bins", "full bins"]:
        assert lmcs.get(name), f"lmcs_scale_chroma: no case with: {name} (have {lmcs})"
    print(seen, cclm, lmcs)

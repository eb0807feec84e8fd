"""CPU: the oracle against the reference decoder's own C path, bit-exactly, slot by slot.

`ref` is oracle/_ref/libvvcref.so (oracle/ref_shim.c linked against the reference's static libraries by `make -C oracle ref`).
Every slot runs its committed case list (tests/ref_cases.py, seed 0) and a wider sweep: rounds of freshly drawn cases (seeds 1, 2, ...)
until at least SWEEP of them are compared.  The helpers of ref_cases.EXHAUSTIVE list their whole domain and have no sweep.
Where the library is absent the comparisons skip; where the reference tree is present and the library is not, one test fails.
Run with -rA (or -s) to see how many cases each slot compared."""
import pytest

import ref_cases
import ref_lib

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
    assert ref_lib.load() is not None, f"the reference tree is at {tree} but {ref_lib.LIB_PATH} is missing: run `make -C oracle ref`"


def compare(orc, ref, slot, seed):
    f_orc, f_ref = getattr(orc, "orc_" + slot), getattr(ref, "ref_" + slot)
    lst = ref_cases.cases(slot, seed)
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


@pytest.mark.parametrize("slot", ["fetch_samples", "avg", "lmcs_filter", "lf_ladf_level", "alf_recon_coeff_and_clip", "intra_wide_angle"])
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

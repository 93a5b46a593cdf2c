"""nts_cigar_alleles (csrc/nts_cigar.inc, Context.cigar_alleles; docs/design/04_32_block_variant_sites.md) against
tests/variant_sites_brute.py: the alleles, allele_first and the carriers of hand-made groups -- the smallest shapes that can go wrong,
the small ones with their records written out --, alleles that one field alone tells apart, 600 chains stacked on one insertion slot, a
1 000-byte insertion that differs in its last byte, groups and emptiness, reference bases beyond 2^32, random groups, and every refusal
with the chain it names.  The alt bytes are opaque to the call: the tests make them up.  Every expectation is computed on the CPU before
the GPU is called.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import variant_sites_brute as VB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, P, EQ, X = 1, 2, 6, 7, 8
SNV, DEL, INS = 1, 2, 3
EINVAL, ERANGE = -22, -34
FIELDS = ("pos", "len", "ref_off", "alt_off", "carrier_first", "group", "kind", "n_carriers")
TIMERS = ("cigar_alleles_events", "cigar_alleles_emit")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    c.profile(True)
    yield c
    c.close()


def as_tuples(alleles):
    return [tuple(int(a[f]) for f in FIELDS) for a in alleles]


def made_up_alts(lists, seed, letters=b"ACGT"):
    "per chain alt bytes of the right length, drawn from `letters`"
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(list(letters), VB.byte_counts(entries)[1]).tolist()) for entries in lists]


def check(ctx, specs, alts, what, n_groups=None):
    "specs: per chain (group, t0, CIGAR string or entries); alts: per chain its alt bytes.  Returns the brute force's (alleles, carriers)"
    from ntsynt_amd.device import CIG_ALLELE_DTYPE
    cigar, recs, lists = arrays([s[2] for s in specs])
    groups = n_groups if n_groups is not None else (specs[-1][0] + 1 if specs else 0)
    want, want_first, want_carriers = VB.alleles([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], alts, groups)
    alt = np.frombuffer(b"".join(alts), dtype=np.uint8)
    alleles, allele_first, carriers = ctx.cigar_alleles(cigar, recs, at_of(specs), alt, n_groups)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {groups} groups, {alt.size} alt bytes -> {alleles.size} alleles, {carriers.size} carriers")
    assert alleles.dtype == CIG_ALLELE_DTYPE and CIG_ALLELE_DTYPE.itemsize == 56 and allele_first.dtype == np.uint64 and carriers.dtype == np.uint32, what
    have = as_tuples(alleles)
    if have != want:
        at = next(i for i in range(max(len(have), len(want))) if have[i:i + 1] != want[i:i + 1])
        raise AssertionError((what, "first difference at", at, have[max(at - 2, 0):at + 3], want[max(at - 2, 0):at + 3]))
    assert allele_first.tolist() == want_first, (what, allele_first.tolist(), want_first)
    assert carriers.tolist() == want_carriers, (what, carriers.tolist()[:20], want_carriers[:20])
    assert not alleles["reserved"].any(), what
    again = ctx.cigar_alleles(cigar, recs, at_of(specs), alt, n_groups)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((alleles, allele_first, carriers), again)), what
    return want, want_carriers


def carriers_of(found, carriers):
    return [carriers[a[4]:a[4] + a[7]] for a in found]


# ---- basic cases: the records are also written out, so that the brute force is checked too ----
#                          pos, len, ref_off, alt_off, carrier_first, group, kind, n_carriers

def test_one_chain_with_an_x_and_a_d(ctx):
    assert check(ctx, [(0, 100, "5=1X2D3=")], [b"G"], "5= 1X 2D 3=") == ([(105, 1, 0, 0, 0, 0, SNV, 1), (106, 2, 1, 0, 1, 0, DEL, 1)], [0, 0])


def test_one_chain_with_an_insertion(ctx):
    assert check(ctx, [(0, 10, "4=2I4=")], [b"AC"], "4= 2I 4=") == ([(14, 2, 0, 0, 0, 0, INS, 1)], [0])


def test_a_split_x_entry_gives_the_same_events(ctx):
    whole = check(ctx, [(0, 0, "3X1=")], [b"ACG"], "3X")
    split = check(ctx, [(0, 0, [1 << 4 | X, 1 << 4 | X, 1 << 4 | X, 1 << 4 | EQ])], [b"ACG"], "1X 1X 1X")
    assert whole == split == ([(0, 1, 0, 0, 0, 0, SNV, 1), (1, 1, 1, 1, 1, 0, SNV, 1), (2, 1, 2, 2, 2, 0, SNV, 1)], [0, 0, 0])


# ---- cases that separate alleles ----

def test_two_chains_with_the_same_snv_are_one_allele(ctx):
    assert check(ctx, [(0, 0, "2=1X2="), (0, 0, "2=1X2=")], [b"T", b"T"], "the same SNV") == ([(2, 1, 0, 0, 0, 0, SNV, 2)], [0, 1])
    found, carriers = check(ctx, [(0, 0, "2=1X2="), (0, 1, "3="), (0, 1, "1=1X2=")], [b"T", b"", b"T"], "the same SNV from different t0")
    assert found == [(2, 1, 0, 0, 0, 0, SNV, 2)] and carriers == [0, 2]


def test_another_alt_byte_at_the_same_position_is_another_allele_in_byte_order(ctx):
    found, carriers = check(ctx, [(0, 0, "2=1X2="), (0, 0, "2=1X2="), (0, 0, "2=1X2=")], [b"T", b"C", b"T"], "T C T")
    assert found == [(2, 1, 1, 1, 0, 0, SNV, 1), (2, 1, 0, 0, 1, 0, SNV, 2)] and carriers == [1, 0, 2]


def test_snv_del_and_ins_at_one_pos_come_in_kind_order(ctx):
    found, _ = check(ctx, [(0, 0, "2=2I3="), (0, 0, "2=3D2="), (0, 0, "2=1X2=")], [b"GG", b"", b"T"], "INS, DEL, SNV at 2")
    assert [(a[0], a[6]) for a in found] == [(2, SNV), (2, DEL), (2, INS)]
    assert found == [(2, 1, 3, 2, 0, 0, SNV, 1), (2, 3, 0, 0, 1, 0, DEL, 1), (2, 2, 0, 0, 2, 0, INS, 1)]


def test_two_deletions_at_one_pos_with_lengths_2_and_5(ctx):
    found, carriers = check(ctx, [(0, 0, "2=5D2="), (0, 0, "2=2D5="), (0, 0, "2=5D2=")], [b"", b"", b""], "5D 2D 5D")
    assert found == [(2, 2, 5, 0, 0, 0, DEL, 1), (2, 5, 0, 0, 1, 0, DEL, 2)] and carriers == [1, 0, 2]


def test_insertions_of_equal_length_at_one_slot_with_bytes_a_b_a(ctx):
    found, carriers = check(ctx, [(0, 0, "2=2I2=")] * 3, [b"AC", b"GT", b"AC"], "A B A")
    assert found == [(2, 2, 0, 0, 0, 0, INS, 2), (2, 2, 0, 2, 2, 0, INS, 1)] and carriers_of(found, carriers) == [[0, 2], [1]]
    found, carriers = check(ctx, [(0, 0, "2=2I2=")] * 3, [b"GT", b"AC", b"AC"], "B A A: the order is the smallest carrier's, not the bytes'")
    assert carriers_of(found, carriers) == [[0], [1, 2]]
    found, carriers = check(ctx, [(0, 0, "1=1X2I2="), (0, 0, "2=2I2="), (0, 0, "1X1=2I2=")], [b"TAC", b"AC", b"GAC"], "the same bytes at offsets 1, 3 and 6")
    assert carriers_of(found, carriers) == [[2], [0], [0, 1, 2]]


# ---- stacked chains ----

def test_600_chains_stacked_on_one_slot_with_three_byte_strings(ctx):
    texts = [b"ACGTACGT", b"ACGTACGA", b"TCGTACGT"]
    found, carriers = check(ctx, [(0, 100, "50=8I50=")] * 600, [texts[c % 3] for c in range(600)], "600 stacked insertions")
    assert [(a[0], a[1], a[6], a[7]) for a in found] == [(150, 8, INS, 200)] * 3
    assert carriers_of(found, carriers) == [list(range(r, 600, 3)) for r in range(3)]


def test_a_1000_byte_insertion_that_differs_in_its_last_byte(ctx):
    long = bytes(np.random.default_rng(1).choice(list(b"ACGT"), 1000).tolist())
    other = long[:-1] + (b"A" if long[-1:] != b"A" else b"C")
    for shift in range(4):                                    # (every alignment of the second chain's bytes against the first's)
        specs = [(0, 0, "4=1000I2="), (0, 0, f"{4 - shift}={shift}X1000I2=" if shift else "4=1000I2="), (0, 0, "4=1000I2=")]
        found, carriers = check(ctx, specs, [long, b"G" * shift + other, long], f"1 000 bytes, shifted by {shift}")
        ins = [a for a in found if a[6] == INS]
        assert [(a[1], a[7]) for a in ins] == [(1000, 2), (1000, 1)] and carriers_of(ins, carriers) == [[0, 2], [1]]
        found, carriers = check(ctx, specs, [long, b"G" * shift + long, other], f"1 000 equal bytes, shifted by {shift}")
        assert carriers_of([a for a in found if a[6] == INS], carriers) == [[0, 1], [2]]


# ---- groups and emptiness ----

def test_two_groups_with_equal_positions_and_an_empty_group_between(ctx):
    specs = [(0, 50, "2=1X2="), (2, 50, "2=1X2="), (2, 50, "2=1X2=")]
    found, carriers = check(ctx, specs, [b"T", b"T", b"T"], "equal positions in two groups", n_groups=4)
    assert found == [(52, 1, 0, 0, 0, 0, SNV, 1), (52, 1, 1, 1, 1, 2, SNV, 2)] and carriers == [0, 1, 2]
    alleles, allele_first, _ = ctx.cigar_alleles(*arrays([s[2] for s in specs])[:2], at_of(specs), np.frombuffer(b"TTT", dtype=np.uint8), 4)
    assert allele_first.tolist() == [0, 1, 1, 2, 2]
    found, _ = check(ctx, specs, [b"T", b"T", b"T"], "n_groups left out: the last chain's group + 1")
    assert len(found) == 2


def test_empty_chains_and_chains_of_equal_alone(ctx):
    specs = [(0, 0, ""), (0, 0, "6=2I6="), (0, 3, ""), (0, 0, ""), (0, 0, "12="), (1, 7, ""), (1, 0, "3=1X3="), (1, 0, "")]
    found, carriers = check(ctx, specs, [b"", b"AA", b"", b"", b"", b"", b"C", b""], "empty chains")
    assert found == [(6, 2, 0, 0, 0, 0, INS, 1), (3, 1, 0, 2, 1, 1, SNV, 1)] and carriers == [1, 6]
    assert check(ctx, [(0, 5, ""), (0, 6, "")], [b"", b""], "only empty chains") == ([], [])
    check(ctx, [(0, 0, "4=1X4=")], [b"A"], "a call with events")
    before = [ctx.timing(t)[1] for t in TIMERS]
    assert check(ctx, [(0, 5, "9="), (1, 6, "120=")], [b"", b""], "= alone: entries, but no event") == ([], [])
    assert [ctx.timing(t)[1] for t in TIMERS] == [before[0] + 2, before[1]], "no event: the stage alone, twice"


def test_no_chain_at_all_launches_nothing(ctx):
    check(ctx, [(0, 0, "4=1X4=")], [b"A"], "a call with events")
    before = [ctx.timing(t)[1] for t in TIMERS]
    assert before[0] > 0 and before[1] > 0
    none = np.zeros(0, dtype=np.uint8)
    for n_groups in (0, 3):
        alleles, allele_first, carriers = ctx.cigar_alleles(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), none, n_groups)
        assert alleles.size == 0 and carriers.size == 0 and allele_first.tolist() == [0] * (n_groups + 1)
    assert [ctx.timing(t)[1] for t in TIMERS] == before, "no chain: nothing is launched"


# ---- wide inputs and repeat calls ----

def test_reference_bases_beyond_2_to_the_32(ctx):
    t0 = (1 << 33) + 5
    found, _ = check(ctx, [(0, t0, "4=1X2="), (0, t0 + 2, "2=1X1D2=")], [b"A", b"A"], "t0 beyond 2^32")
    assert found == [(t0 + 4, 1, 0, 0, 0, 0, SNV, 2), (t0 + 5, 1, 2, 0, 2, 0, DEL, 1)]


def test_300_random_chains_in_40_groups(ctx):
    specs = random_groups(5, 300, 40)
    lists = arrays([s[2] for s in specs])[2]
    found, _ = check(ctx, specs, made_up_alts(lists, 7, b"AC"), "300 random chains", n_groups=40)
    assert len(found) > 300 and {a[6] for a in found} == {SNV, DEL, INS} and any(a[7] > 1 for a in found) and any(a[0] > 1 << 32 for a in found)
    specs = random_groups(6, 300, 40)
    check(ctx, specs, made_up_alts(arrays([s[2] for s in specs])[2], 8), "300 other random chains", n_groups=40)


# ---- refusals ----

def raw_call(ctx, cigar, recs, at, n_groups, alt, allele_first, n_cigar=None, n_chains=None, n_alt=None):
    "the C call itself, with sizes that need not be the arrays': (return code, the two pointers and the count as the call left them)"
    mark = 0x5A5A5A5A
    p_alleles, p_carriers, n_carriers = ctypes.c_void_p(mark), ctypes.c_void_p(mark), ctypes.c_uint64(mark)
    rc = ctx.lib.nts_cigar_alleles(ctx.h, cigar.ctypes.data, cigar.size if n_cigar is None else n_cigar, recs.ctypes.data,
                                   recs.size if n_chains is None else n_chains, at.ctypes.data, n_groups, alt.ctypes.data if alt.size else None,
                                   alt.size if n_alt is None else n_alt, ctypes.byref(p_alleles), allele_first.ctypes.data, ctypes.byref(p_carriers),
                                   ctypes.byref(n_carriers))
    return rc, (p_alleles.value, p_carriers.value, n_carriers.value) == (mark, mark, mark)


def refused(ctx, specs, code, words, n_groups=None, mutate=None, alts=None):
    from ntsynt_amd.device import NtsError
    cigar, recs, lists = arrays([s[2] for s in specs])
    alt = np.frombuffer(b"".join(alts if alts is not None else made_up_alts(lists, 3)), dtype=np.uint8)
    if mutate:
        mutate(cigar, recs)
    with pytest.raises(NtsError) as err:
        ctx.cigar_alleles(cigar, recs, at_of(specs), alt, n_groups)
    assert f"(code {code})" in str(err.value) and "nts_cigar_alleles" in str(err.value) and all(w in str(err.value) for w in words), \
        (code, words, str(err.value))


def test_refusals_name_the_smallest_offending_chain(ctx):
    good = (0, 0, "4=1I4=")
    refused(ctx, [good, (1, 0, "4="), (0, 0, "4="), (0, 0, "1I4=")], EINVAL, ["chain 2", "nondecreasing"], n_groups=2)
    refused(ctx, [good, good, (2, 0, "4="), (3, 0, "4=")], EINVAL, ["chain 2", "n_groups"], n_groups=2)
    refused(ctx, [good, (0, 0, "1I4="), (0, 0, "2D4=")], EINVAL, ["chain 1", "first or last entry is not = or X"])
    refused(ctx, [good, (0, 0, "4=2D"), (0, 0, "2D4=")], EINVAL, ["chain 1", "first or last entry is not = or X"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | P, 4 << 4 | EQ]), (0, 0, [1 << 4 | EQ, 1 << 4 | P, 1 << 4 | X])], EINVAL, ["chain 1", "code 6"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | 3, 4 << 4 | EQ]), (0, 0, [1 << 4 | EQ, 2 << 4 | 3, 1 << 4 | EQ])], EINVAL,
            ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 0 << 4 | D, 4 << 4 | EQ])], EINVAL, ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 1 << 32, "4="), (0, 1 << 33, "4=")], ERANGE, ["chain 1", "2^32"])
    refused(ctx, [good, (0, (1 << 64) - 2, "4="), (0, (1 << 64) - 1, "4=")], ERANGE, ["chain 1", "wraps"])

    def long(cigar, recs):
        recs["len_a"][1] = 1 << 62
    refused(ctx, [good, (0, 0, "4=")], ERANGE, ["2^62 bases or more"], mutate=long)

    def shift(cigar, recs):
        recs["first"][1] += 1
    refused(ctx, [good, (0, 0, "4="), (0, 0, "4=")], EINVAL, ["chain 1", "tile"], mutate=shift)

    def short(cigar, recs):
        recs["len_a"][1] -= 1
    refused(ctx, [good, (0, 0, "4=2D1="), (0, 0, "4=")], EINVAL, ["chain 1", "no CIGAR of its lengths"], mutate=short)
    check(ctx, [good, (0, (1 << 32) - 9, "4=")], [b"A", b""], "an extent of 2^32 - 1 - 4 bases passes")


def test_an_alt_buffer_of_another_length_is_refused(ctx):
    specs = [(0, 0, "4=1I4="), (0, 0, "2=2X1=")]
    refused(ctx, specs, EINVAL, ["alt holds 2 bytes, the X and I entries of the chains have 3"], alts=[b"A", b"C"])
    refused(ctx, specs, EINVAL, ["alt holds 4 bytes, the X and I entries of the chains have 3"], alts=[b"A", b"CGT"])
    refused(ctx, specs, EINVAL, ["alt holds 0 bytes, the X and I entries of the chains have 3"], alts=[b"", b""])
    refused(ctx, [(0, 0, "4=")], EINVAL, ["alt holds 1 bytes, the X and I entries of the chains have 0"], alts=[b"A"])
    refused(ctx, [], EINVAL, ["alt holds 1 bytes, the X and I entries of the chains have 0"], alts=[b"A"], n_groups=1)
    check(ctx, specs, [b"A", b"CG"], "the right length passes")


def test_2_to_the_32_entries_chains_or_groups_are_refused_before_any_array_is_read(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays(["4="])
    at = at_of([(0, 0, 0)])
    for sizes in (dict(n_cigar=1 << 32), dict(n_chains=1 << 32), dict(n_groups=1 << 32)):
        allele_first = np.full(2, 0xABABABABABABABAB, dtype=np.uint64)
        rc, untouched = raw_call(ctx, cigar, recs, at, sizes.pop("n_groups", 1), np.zeros(0, dtype=np.uint8), allele_first, **sizes)
        assert rc == ERANGE and untouched and allele_first.tolist() == [0xABABABABABABABAB] * 2, sizes
        with pytest.raises(NtsError) as err:
            ctx.check(rc, "nts_cigar_alleles")
        assert "2^32 entries, chains or groups or more" in str(err.value)


def test_a_refused_call_leaves_the_outputs_as_passed_in(ctx):
    for specs, alt, n_groups, code in (([(0, 0, "4="), (0, 0, [4 << 4 | EQ, 2 << 4 | P, 1 << 4 | EQ])], b"", 1, EINVAL),     # behind the first scan
                                       ([(0, 0, "4="), (0, 0, [1 << 4 | EQ, 2 << 4 | 5, 1 << 4 | EQ])], b"", 1, EINVAL),     # behind the first scan
                                       ([(0, 0, "2=1X1="), (0, 0, "2=2I1=")], b"AC", 1, EINVAL),                            # behind the first scan: alt
                                       ([(1, 0, "4="), (0, 0, "4=")], b"", 2, EINVAL),                                       # before any launch
                                       ([(0, 0, "4="), (0, 0, "2I4=")], b"AC", 1, EINVAL),                                   # before any launch
                                       ([(0, 0, "4="), (0, 1 << 32, "4=")], b"", 1, ERANGE)):
        cigar, recs, _ = arrays([s[2] for s in specs])
        allele_first = np.full(n_groups + 1, 0xABABABABABABABAB, dtype=np.uint64)
        rc, untouched = raw_call(ctx, cigar, recs, at_of(specs), n_groups, np.frombuffer(alt, dtype=np.uint8), allele_first)
        assert rc == code and untouched and allele_first.tolist() == [0xABABABABABABABAB] * (n_groups + 1), specs
    assert check(ctx, [(0, 0, "2=1X1=")], [b"G"], "the context still answers") == ([(2, 1, 0, 0, 0, 0, SNV, 1)], [0])

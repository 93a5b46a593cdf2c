"""nts_cigar_profile (csrc/nts_cigar.inc, Context.cigar_profile; docs/design/04_33_block_consensus.md) against tests/profile_brute.py:
the columns and col_first of hand-made groups -- the smallest shapes that can go wrong, the small ones with their records written out --,
every tie of the call, insertions of different lengths in one slot, foreign sites at a chain's first and last base, split entries,
overlaps, holes, groups and emptiness, 600 chains stacked on one column and on one slot, a long deletion under 600 chains, bytes that are
no base, reference bases beyond 2^32, random groups, and every refusal with the chain it names.  The ref and alt bytes are opaque to the
call: the tests make them up.  Every expectation is computed on the CPU before the GPU is called.  Every test runs under a time limit of
its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import profile_brute as PB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, P, EQ, X = 1, 2, 6, 7, 8
REF = PB.REF
EINVAL, ERANGE = -22, -34
TIMERS = ("cigar_profile_events", "cigar_profile_emit")
NONE = (0, 0, 0, 0, 0)


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


def made_up(lists, seed, letters=b"ACGT"):
    "per chain (ref bytes, alt bytes) of the right lengths, drawn from `letters`"
    rng = np.random.default_rng(seed)
    return ([bytes(rng.choice(list(letters), PB.byte_counts(entries)[0]).tolist()) for entries in lists],
            [bytes(rng.choice(list(letters), PB.byte_counts(entries)[1]).tolist()) for entries in lists])


def check(ctx, specs, refs, alts, what, n_groups=None):
    "specs: per chain (group, t0, CIGAR string or entries); refs, alts: per chain its bytes.  Returns the brute force's columns"
    from ntsynt_amd.device import CIG_PROFILE_COL_DTYPE
    cigar, recs, lists = arrays([s[2] for s in specs])
    groups = n_groups if n_groups is not None else (specs[-1][0] + 1 if specs else 0)
    want, want_first = PB.columns([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], refs, alts, groups)
    ref, alt = np.frombuffer(b"".join(refs), dtype=np.uint8), np.frombuffer(b"".join(alts), dtype=np.uint8)
    cols, col_first = ctx.cigar_profile(cigar, recs, at_of(specs), ref, alt, n_groups)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {groups} groups, {ref.size} ref and {alt.size} alt bytes -> {cols.size} columns")
    assert cols.dtype == CIG_PROFILE_COL_DTYPE and CIG_PROFILE_COL_DTYPE.itemsize == 56 and col_first.dtype == np.uint64, what
    have = PB.as_tuples(cols)
    if have != want:
        at = next(i for i in range(max(len(have), len(want))) if have[i:i + 1] != want[i:i + 1])
        raise AssertionError((what, "first difference at", at, have[max(at - 2, 0):at + 3], want[max(at - 2, 0):at + 3]))
    assert col_first.tolist() == want_first, (what, col_first.tolist(), want_first)
    assert not cols["reserved"].any(), what
    again = ctx.cigar_profile(cigar, recs, at_of(specs), ref, alt, n_groups)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((cols, col_first), again)), what
    return want


# ---- basic cases: the records are also written out, so that the brute force is checked too ----
#             pos, group, sub, aligned, match, gap, n (A C G T N), ref, call

def test_one_chain_with_an_x_and_a_d(ctx):
    got = check(ctx, [(0, 100, "5=1X2D3=")], [b"ATG"], [b"G"], "5= 1X 2D 3=")
    assert got == [(105, 0, REF, 1, 0, 0, (0, 0, 1, 0, 0), "A", "A"),       # A 1 : G 1, the reference wins
                   (106, 0, REF, 1, 0, 1, NONE, "T", "T"),                  # T 1 : - 1, the base wins
                   (107, 0, REF, 1, 0, 1, NONE, "G", "G")]


def test_the_same_x_under_three_chains(ctx):
    specs = [(0, 100, "5=1X5=")] * 3
    assert check(ctx, specs, [b"A"] * 3, [b"G"] * 3, "three chains, one alt byte") == [(105, 0, REF, 3, 0, 0, (0, 0, 3, 0, 0), "A", "G")]
    assert check(ctx, specs[:2], [b"A"] * 2, [b"G", b"C"], "two chains, two alt bytes") == [(105, 0, REF, 2, 0, 0, (0, 1, 1, 0, 0), "A", "A")]
    specs = [(0, 100, "5=1X5="), (0, 100, "5=1X5="), (0, 100, "11=")]
    assert check(ctx, specs, [b"A", b"A", b""], [b"G", b"C", b""], "two alt bytes and a match") == [(105, 0, REF, 3, 1, 0, (0, 1, 1, 0, 0), "A", "A")]
    assert check(ctx, specs, [b"A", b"A", b""], [b"G", b"G", b""], "G 2 : A 2, the reference wins") == [(105, 0, REF, 3, 1, 0, (0, 0, 2, 0, 0), "A", "A")]


def test_ties_the_reference_is_no_part_of(ctx):
    specs = [(0, 0, "2=1X2=")] * 4
    assert check(ctx, specs[:3], [b"A"] * 3, [b"C", b"C", b"G"], "C C G over A") == [(2, 0, REF, 3, 0, 0, (0, 2, 1, 0, 0), "A", "C")]
    assert check(ctx, specs, [b"A"] * 4, [b"G", b"G", b"C", b"C"], "G G C C over A: C by order") == [(2, 0, REF, 4, 0, 0, (0, 2, 2, 0, 0), "A", "C")]
    assert check(ctx, specs, [b"C"] * 4, [b"T", b"G", b"T", b"G"], "T G T G over C: G by order") == [(2, 0, REF, 4, 0, 0, (0, 0, 2, 2, 0), "C", "G")]


def test_insertions_of_3_and_5_bytes_in_one_slot(ctx):
    specs = [(0, 100, "4=3I4="), (0, 100, "4=5I4="), (0, 100, "8=")]
    got = check(ctx, specs, [b"", b"", b""], [b"ACG", b"ACGTT", b""], "I 3 and I 5 under a third chain")
    assert got == [(104, 0, 0, 3, 0, 1, (2, 0, 0, 0, 0), "-", "-"), (104, 0, 1, 3, 0, 1, (0, 2, 0, 0, 0), "-", "-"),     # 2 : 2 against -, - wins
                   (104, 0, 2, 3, 0, 1, (0, 0, 2, 0, 0), "-", "-"), (104, 0, 3, 3, 0, 2, (0, 0, 0, 1, 0), "-", "-"),
                   (104, 0, 4, 3, 0, 2, (0, 0, 0, 1, 0), "-", "-")]
    got = check(ctx, specs + [(0, 100, "4=3I4=")], [b""] * 4, [b"ACG", b"ACGTT", b"", b"ACG"], "a fourth chain that carries the bytes")
    assert [(c[2], c[3], c[5], c[8]) for c in got] == [(0, 4, 1, "A"), (1, 4, 1, "C"), (2, 4, 1, "G"), (3, 4, 3, "-"), (4, 4, 3, "-")]
    got = check(ctx, specs + [(0, 100, "4=3I4=")], [b""] * 4, [b"ACG", b"ATGTT", b"", b"ACG"], "the bytes differ in column 1")
    assert got[1] == (104, 0, 1, 4, 0, 1, (0, 2, 0, 1, 0), "-", "-") and got[0][8] == "A"       # C 2 : T 1 : - 2, - wins the tie
    got = check(ctx, [(0, 100, "4=2I4="), (0, 100, "4=2I4=")], [b"", b""], [b"AC", b"AG"], "two holders alone: 1 : 1 : 1 in column 1")
    assert [(c[2], c[6], c[8]) for c in got] == [(0, (2, 0, 0, 0, 0), "A"), (1, (0, 1, 1, 0, 0), "-")]


def test_foreign_sites_at_the_first_base_the_last_base_and_inside_a_deletion(ctx):
    # chain 0 holds an insertion in slot 10 and an X at 20; chain 1 begins at 10 (covers slot 10: a gap), chain 2 ends at 10 (does not),
    # chain 3 begins at 20, chain 4 ends at 20, chain 5 deletes 8 .. 12 (slot 10 inside its D: covered, a gap)
    specs = [(0, 0, "10=2I10=1X9="), (0, 10, "5="), (0, 5, "5="), (0, 20, "3="), (0, 17, "3="), (0, 6, "2=4D2=")]
    got = check(ctx, specs, [b"T", b"", b"", b"", b"", b"CCCC"], [b"GGA", b"", b"", b"", b"", b""], "foreign sites")
    slot = [c for c in got if c[0] == 10 and c[2] != REF]
    assert slot == [(10, 0, 0, 3, 0, 2, (0, 0, 1, 0, 0), "-", "-"), (10, 0, 1, 3, 0, 2, (0, 0, 1, 0, 0), "-", "-")]
    assert [c for c in got if c[0] == 20] == [(20, 0, REF, 2, 1, 0, (1, 0, 0, 0, 0), "T", "T")]
    assert [c for c in got if c[0] == 10 and c[2] == REF] == [(10, 0, REF, 3, 2, 1, NONE, "C", "C")]


def test_an_own_insertion_followed_by_a_deletion(ctx):
    got = check(ctx, [(0, 50, "3=2I2D3="), (0, 50, "8=")], [b"AC", b""], [b"GG", b""], "2I 2D")
    assert [(c[0], c[2], c[3], c[5], c[8]) for c in got] == [(53, 0, 2, 1, "-"), (53, 1, 2, 1, "-"), (53, REF, 2, 1, "A"), (54, REF, 2, 1, "C")]


def test_split_x_and_d_entries_equal_the_merged_ones(ctx):
    other = (0, 0, "4=1X1=1D5=")
    whole = check(ctx, [(0, 0, "2=5X3D2="), other], [b"ACGTACGT", b"GT"], [b"TTTTT", b"A"], "5X 3D")
    split = check(ctx, [(0, 0, [2 << 4 | EQ, 3 << 4 | X, 2 << 4 | X, 2 << 4 | D, 1 << 4 | D, 2 << 4 | EQ]), other], [b"ACGTACGT", b"GT"], [b"TTTTT", b"A"],
                  "3X 2X 2D 1D")
    assert whole == split and len(whole) == 8


def test_two_chains_overlapping_in_the_middle_in_either_order_and_a_hole(ctx):
    a, b = (0, 100, "6=1X3="), (0, 104, "2=1X1D4=")
    first = check(ctx, [a, b], [b"A", b"AC"], [b"T", b"G"], "a then b")
    second = check(ctx, [b, a], [b"AC", b"A"], [b"G", b"T"], "b then a")
    assert [c[:7] + c[8:] for c in first] == [c[:7] + c[8:] for c in second]
    assert first == [(106, 0, REF, 2, 0, 0, (0, 0, 1, 1, 0), "A", "A"), (107, 0, REF, 2, 1, 1, NONE, "C", "C")]
    got = check(ctx, [(0, 0, "2=1X2="), (0, 100, "2=1X2=")], [b"A", b"C"], [b"G", b"T"], "a hole between two chains")
    assert [(c[0], c[3]) for c in got] == [(2, 1), (102, 1)]


# ---- groups and emptiness ----

def test_two_groups_with_equal_positions_and_an_empty_group_between(ctx):
    specs = [(0, 50, "2=1X2="), (2, 50, "2=1X2="), (2, 50, "2=1X2=")]
    got = check(ctx, specs, [b"A"] * 3, [b"T"] * 3, "equal positions in two groups", n_groups=4)
    assert got == [(52, 0, REF, 1, 0, 0, (0, 0, 0, 1, 0), "A", "A"), (52, 2, REF, 2, 0, 0, (0, 0, 0, 2, 0), "A", "T")]
    _, col_first = ctx.cigar_profile(*arrays([s[2] for s in specs])[:2], at_of(specs), np.frombuffer(b"AAA", dtype=np.uint8),
                                     np.frombuffer(b"TTT", dtype=np.uint8), 4)
    assert col_first.tolist() == [0, 1, 1, 2, 2]
    assert len(check(ctx, specs, [b"A"] * 3, [b"T"] * 3, "n_groups left out: the last chain's group + 1")) == 2


def test_empty_chains_and_chains_of_equal_alone(ctx):
    specs = [(0, 0, ""), (0, 0, "6=2I6="), (0, 3, ""), (0, 0, ""), (0, 0, "12="), (1, 7, ""), (1, 0, "3=1X3="), (1, 0, "")]
    got = check(ctx, specs, [b""] * 6 + [b"G", b""], [b"", b"AA", b"", b"", b"", b"", b"C", b""], "empty chains")
    assert got == [(6, 0, 0, 2, 0, 1, (1, 0, 0, 0, 0), "-", "-"), (6, 0, 1, 2, 0, 1, (1, 0, 0, 0, 0), "-", "-"), (3, 1, REF, 1, 0, 0, (0, 1, 0, 0, 0), "G", "G")]
    assert check(ctx, [(0, 5, ""), (0, 6, "")], [b"", b""], [b"", b""], "only empty chains") == []
    check(ctx, [(0, 0, "4=1X4=")], [b"C"], [b"A"], "a call with events")
    before = [ctx.timing(t)[1] for t in TIMERS]
    assert check(ctx, [(0, 5, "9="), (1, 6, "120=")], [b"", b""], [b"", b""], "= alone: entries, but no event") == []
    assert [ctx.timing(t)[1] for t in TIMERS] == [before[0] + 2, before[1]], "no event: the stage alone, twice"
    assert check(ctx, [(0, 7, "3=1X2=")], [b"T"], [b"A"], "one chain") == [(10, 0, REF, 1, 0, 0, (1, 0, 0, 0, 0), "T", "T")]


def test_no_chain_at_all_launches_nothing(ctx):
    check(ctx, [(0, 0, "4=1X4=")], [b"C"], [b"A"], "a call with events")
    before = [ctx.timing(t)[1] for t in TIMERS]
    assert before[0] > 0 and before[1] > 0
    none = np.zeros(0, dtype=np.uint8)
    for n_groups in (0, 3):
        cols, col_first = ctx.cigar_profile(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), none, none, n_groups)
        assert cols.size == 0 and col_first.tolist() == [0] * (n_groups + 1)
    assert [ctx.timing(t)[1] for t in TIMERS] == before, "no chain: nothing is launched"


# ---- larger stacks ----

def test_600_chains_stacked_on_one_x_column(ctx):
    got = check(ctx, [(0, 100, "50=1X50=")] * 600, [b"A"] * 600, [b"ACGTN"[c % 5:c % 5 + 1] for c in range(600)], "600 stacked X columns")
    assert got == [(150, 0, REF, 600, 0, 0, (120,) * 5, "A", "A")]       # A 121 with the reference row
    got = check(ctx, [(0, 100, "50=1X50=")] * 600, [b"G"] * 600, [b"ACTTN"[c % 5:c % 5 + 1] for c in range(600)], "600 stacked X columns, T twice")
    assert got == [(150, 0, REF, 600, 0, 0, (120, 120, 0, 240, 120), "G", "T")]


def test_600_insertions_of_lengths_1_to_600_in_one_slot(ctx):
    alts = [(b"ACGT" * 150)[:n] for n in range(1, 601)]
    got = check(ctx, [(0, 10, f"5={n}I5=") for n in range(1, 601)], [b""] * 600, alts, "600 insertions of lengths 1 .. 600")
    assert len(got) == 600 and all(c[2] == i and c[3] == 600 and sum(c[6]) == 600 - i and c[5] == i for i, c in enumerate(got))
    assert [c[8] for c in got[:300]] == list("ACGT" * 75) and got[300][8] == "-" and got[599][8] == "-"     # column 299: 301 : 300, column 300: 300 : 301


def test_one_d_entry_of_20000_bases_under_600_one_base_chains(ctx):
    specs = [(0, 0, "5=20000D5=")] + [(0, 5 + 33 * c, "1=") for c in range(600)]
    got = check(ctx, specs, [b"ACGT" * 5000] + [b""] * 600, [b""] * 601, "a long deletion")
    assert len(got) == 20000 and [c[0] for c in got] == list(range(5, 20005))
    assert all(c[3] == (2 if (c[0] - 5) % 33 == 0 and c[0] < 5 + 33 * 600 else 1) and c[5] == 1 and c[4] == c[3] - 1 for c in got)
    assert all(c[8] == c[7] == "ACGT"[(c[0] - 5) % 4] for c in got)


def test_bytes_outside_acgtn_count_under_n(ctx):
    got = check(ctx, [(0, 0, "2=1X1=1I2=")] * 3, [b"R"] * 3, [b"a*", b"Y-", b"NN"], "bytes that are no base in alt and ref")
    assert got == [(2, 0, REF, 3, 0, 0, (0, 0, 0, 0, 3), "R", "N"), (4, 0, 0, 3, 0, 0, (0, 0, 0, 0, 3), "-", "N")]
    got = check(ctx, [(0, 0, "2=1X2=")] * 2, [b"n", b"n"], [b"A", b"C"], "a reference byte that is no base counts under N")
    assert got == [(2, 0, REF, 2, 0, 0, (1, 1, 0, 0, 0), "n", "N")]


def test_reference_bases_beyond_2_to_the_32(ctx):
    t0 = (1 << 33) + 5
    got = check(ctx, [(0, t0, "4=1X2="), (0, t0 + 2, "2=1X1D1I2=")], [b"A", b"AC"], [b"G", b"GT"], "t0 beyond 2^32")
    assert [(c[0], c[2]) for c in got] == [(t0 + 4, REF), (t0 + 5, REF), (t0 + 6, 0)] and got[0][6] == (0, 0, 2, 0, 0) and got[0][8] == "G"


def test_300_random_chains_in_40_groups(ctx):
    specs = random_groups(5, 300, 40)
    lists = arrays([s[2] for s in specs])[2]
    got = check(ctx, specs, *made_up(lists, 7, b"AC"), "300 random chains", n_groups=40)
    assert len(got) > 300 and any(c[2] != REF and c[2] > 0 for c in got) and any(c[8] != c[7] for c in got) and any(c[0] > 1 << 32 for c in got)
    specs = random_groups(6, 300, 40)
    check(ctx, specs, *made_up(arrays([s[2] for s in specs])[2], 8, b"ACGTN"), "300 other random chains", n_groups=40)


# ---- refusals ----

def raw_call(ctx, cigar, recs, at, n_groups, ref, alt, col_first, n_cigar=None, n_chains=None):
    "the C call itself, with sizes that need not be the arrays': (return code, whether the pointer is as passed in)"
    mark = 0x5A5A5A5A
    p_cols = ctypes.c_void_p(mark)
    rc = ctx.lib.nts_cigar_profile(ctx.h, cigar.ctypes.data, cigar.size if n_cigar is None else n_cigar, recs.ctypes.data,
                                   recs.size if n_chains is None else n_chains, at.ctypes.data, n_groups, ref.ctypes.data if ref.size else None, ref.size,
                                   alt.ctypes.data if alt.size else None, alt.size, ctypes.byref(p_cols), col_first.ctypes.data)
    return rc, p_cols.value == mark


def refused(ctx, specs, code, words, n_groups=None, mutate=None, refs=None, alts=None):
    from ntsynt_amd.device import NtsError
    cigar, recs, lists = arrays([s[2] for s in specs])
    made = made_up(lists, 3)
    ref = np.frombuffer(b"".join(refs if refs is not None else made[0]), dtype=np.uint8)
    alt = np.frombuffer(b"".join(alts if alts is not None else made[1]), dtype=np.uint8)
    if mutate:
        mutate(cigar, recs)
    with pytest.raises(NtsError) as err:
        ctx.cigar_profile(cigar, recs, at_of(specs), ref, alt, n_groups)
    assert f"(code {code})" in str(err.value) and "nts_cigar_profile" in str(err.value) and all(w in str(err.value) for w in words), \
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
    check(ctx, [good, (0, (1 << 32) - 9, "4=")], [b"", b""], [b"A", b""], "an extent of 2^32 - 1 - 4 bases passes")


def test_byte_buffers_of_another_length_are_refused(ctx):
    specs = [(0, 0, "4=1I4="), (0, 0, "2=2X1D1=")]
    refused(ctx, specs, EINVAL, ["alt holds 2 bytes, the X and I entries of the chains have 3"], refs=[b"", b"ACG"], alts=[b"A", b"C"])
    refused(ctx, specs, EINVAL, ["alt holds 4 bytes, the X and I entries of the chains have 3"], refs=[b"", b"ACG"], alts=[b"A", b"CGT"])
    refused(ctx, specs, EINVAL, ["ref holds 2 bytes, the X and D entries of the chains have 3"], refs=[b"", b"AC"], alts=[b"A", b"CG"])
    refused(ctx, specs, EINVAL, ["ref holds 0 bytes, the X and D entries of the chains have 3"], refs=[b"", b""], alts=[b"A", b"CG"])
    refused(ctx, [(0, 0, "4=")], EINVAL, ["alt holds 1 bytes, the X and I entries of the chains have 0"], refs=[b""], alts=[b"A"])
    refused(ctx, [(0, 0, "4=")], EINVAL, ["ref holds 1 bytes, the X and D entries of the chains have 0"], refs=[b"A"], alts=[b""])
    refused(ctx, [], EINVAL, ["ref holds 1 bytes, the X and D entries of the chains have 0"], refs=[b"A"], alts=[], n_groups=1)
    check(ctx, specs, [b"", b"ACG"], [b"A", b"CG"], "the right lengths pass")


def test_2_to_the_32_entries_chains_or_groups_are_refused_before_any_array_is_read(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays(["4="])
    at = at_of([(0, 0, 0)])
    none = np.zeros(0, dtype=np.uint8)
    for sizes in (dict(n_cigar=1 << 32), dict(n_chains=1 << 32), dict(n_groups=1 << 32)):
        col_first = np.full(2, 0xABABABABABABABAB, dtype=np.uint64)
        rc, untouched = raw_call(ctx, cigar, recs, at, sizes.pop("n_groups", 1), none, none, col_first, **sizes)
        assert rc == ERANGE and untouched and col_first.tolist() == [0xABABABABABABABAB] * 2, sizes
        with pytest.raises(NtsError) as err:
            ctx.check(rc, "nts_cigar_profile")
        assert "2^32 entries, chains or groups or more" in str(err.value)


def test_a_refused_call_leaves_the_outputs_as_passed_in(ctx):
    for specs, ref, alt, n_groups, code in (([(0, 0, "4="), (0, 0, [4 << 4 | EQ, 2 << 4 | P, 1 << 4 | EQ])], b"", b"", 1, EINVAL),     # behind the first scan
                                            ([(0, 0, "4="), (0, 0, [1 << 4 | EQ, 2 << 4 | 5, 1 << 4 | EQ])], b"", b"", 1, EINVAL),     # behind the first scan
                                            ([(0, 0, "2=1X1="), (0, 0, "2=2I1=")], b"A", b"AC", 1, EINVAL),                            # behind the first scan: alt
                                            ([(0, 0, "2=1X1="), (0, 0, "2=2D1=")], b"AC", b"A", 1, EINVAL),                            # behind the first scan: ref
                                            ([(1, 0, "4="), (0, 0, "4=")], b"", b"", 2, EINVAL),                                       # before any launch
                                            ([(0, 0, "4="), (0, 0, "2I4=")], b"", b"AC", 1, EINVAL),                                   # before any launch
                                            ([(0, 0, "4="), (0, 1 << 32, "4=")], b"", b"", 1, ERANGE)):
        cigar, recs, _ = arrays([s[2] for s in specs])
        col_first = np.full(n_groups + 1, 0xABABABABABABABAB, dtype=np.uint64)
        rc, untouched = raw_call(ctx, cigar, recs, at_of(specs), n_groups, np.frombuffer(ref, dtype=np.uint8), np.frombuffer(alt, dtype=np.uint8), col_first)
        assert rc == code and untouched and col_first.tolist() == [0xABABABABABABABAB] * (n_groups + 1), specs
    assert check(ctx, [(0, 0, "2=1X1=")], [b"C"], [b"G"], "the context still answers") == [(2, 0, REF, 1, 0, 0, (0, 0, 1, 0, 0), "C", "C")]

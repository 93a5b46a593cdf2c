"""nts_cigar_depth (csrc/nts_cigar.inc, Context.cigar_depth; docs/design/04_31_block_conservation.md) against
tests/conservation_brute.py: the segments and seg_first of hand-made groups -- the smallest shapes that can go wrong --, the counts
beyond one byte, a run crossed by many boundaries, reference bases beyond 2^32, random groups, and every refusal with the chain it
names.  Every expectation is computed on the CPU before the GPU is called.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import conservation_brute as CB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, P, EQ, X = 1, 2, 6, 7, 8
EINVAL, ERANGE = -22, -34


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


def as_tuples(segs):
    return [tuple(int(s[f]) for f in ("start", "end", "group", "aligned", "match", "gap")) for s in segs]


def check(ctx, specs, what, n_groups=None):
    "specs: per chain (group, t0, CIGAR string or entries).  Returns the brute force's segments"
    from ntsynt_amd.device import CIG_DEPTH_SEG_DTYPE
    cigar, recs, lists = arrays([s[2] for s in specs])
    groups = n_groups if n_groups is not None else (specs[-1][0] + 1 if specs else 0)
    want, want_first = CB.segments([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], groups)
    segs, seg_first = ctx.cigar_depth(cigar, recs, at_of(specs), n_groups)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {groups} groups -> {segs.size} segments")
    assert segs.dtype == CIG_DEPTH_SEG_DTYPE and CIG_DEPTH_SEG_DTYPE.itemsize == 32 and seg_first.dtype == np.uint64, what
    have = as_tuples(segs)
    if have != want:
        at = next(i for i in range(max(len(have), len(want))) if have[i:i + 1] != want[i:i + 1])
        raise AssertionError((what, "first difference at", at, have[max(at - 2, 0):at + 3], want[max(at - 2, 0):at + 3]))
    assert seg_first.tolist() == want_first, (what, seg_first.tolist(), want_first)
    again = ctx.cigar_depth(cigar, recs, at_of(specs), n_groups)
    assert segs.tobytes() == again[0].tobytes() and seg_first.tobytes() == again[1].tobytes(), what
    return want


# ---- one group: the expectation is also written out, so that the brute force is checked too ----

def test_one_chain_with_every_consuming_code(ctx):
    assert check(ctx, [(0, 100, "5=1X2D3=")], "5= 1X 2D 3=") == [(100, 105, 0, 1, 1, 0), (105, 106, 0, 1, 0, 0), (106, 108, 0, 1, 0, 1),
                                                                  (108, 111, 0, 1, 1, 0)]


def test_an_insertion_does_not_split_a_segment(ctx):
    assert check(ctx, [(0, 10, "4=2I4=")], "4= 2I 4=") == [(10, 18, 0, 1, 1, 0)]
    assert check(ctx, [(0, 10, "4=2I1I4=3I")], "neighbouring and trailing I") == [(10, 18, 0, 1, 1, 0)]


def test_entries_that_are_no_maximal_runs(ctx):
    assert check(ctx, [(0, 0, [3 << 4 | X, 2 << 4 | X])], "3X 2X") == [(0, 5, 0, 1, 0, 0)]
    assert check(ctx, [(0, 0, [3 << 4 | EQ, 2 << 4 | EQ, 1 << 4 | D, 4 << 4 | D, 1 << 4 | EQ])], "3= 2= 1D 4D 1=") == \
        [(0, 5, 0, 1, 1, 0), (5, 10, 0, 1, 0, 1), (10, 11, 0, 1, 1, 0)]


def test_a_chain_that_is_no_core(ctx):
    assert check(ctx, [(0, 5, "2D3=1D")], "a leading and a trailing D") == [(5, 7, 0, 1, 0, 1), (7, 10, 0, 1, 1, 0), (10, 11, 0, 1, 0, 1)]
    assert check(ctx, [(0, 5, "2I2D3=1D1I")], "I and D at both ends") == [(5, 7, 0, 1, 0, 1), (7, 10, 0, 1, 1, 0), (10, 11, 0, 1, 0, 1)]


def test_two_chains_that_overlap_in_the_middle(ctx):
    assert check(ctx, [(0, 0, "10="), (0, 5, "10X")], "an overlap") == [(0, 5, 0, 1, 1, 0), (5, 10, 0, 2, 1, 0), (10, 15, 0, 1, 0, 0)]
    assert check(ctx, [(0, 5, "10X"), (0, 0, "10=")], "the same, the later chain first") == [(0, 5, 0, 1, 1, 0), (5, 10, 0, 2, 1, 0), (10, 15, 0, 1, 0, 0)]
    assert check(ctx, [(0, 0, "4=4D4="), (0, 2, "4=4D4=")], "shifted copies") == \
        [(0, 2, 0, 1, 1, 0), (2, 4, 0, 2, 2, 0), (4, 6, 0, 2, 1, 1), (6, 8, 0, 2, 0, 2), (8, 10, 0, 2, 1, 1), (10, 12, 0, 2, 2, 0), (12, 14, 0, 1, 1, 0)]


def test_a_chain_that_ends_where_another_begins(ctx):
    assert check(ctx, [(0, 0, "5="), (0, 5, "5=")], "equal triples on both sides") == [(0, 10, 0, 1, 1, 0)]
    assert check(ctx, [(0, 0, "5="), (0, 5, "5X")], "different triples") == [(0, 5, 0, 1, 1, 0), (5, 10, 0, 1, 0, 0)]
    assert check(ctx, [(0, 0, "9="), (0, 0, "5="), (0, 5, "4=")], "under a third chain") == [(0, 9, 0, 2, 2, 0)]


def test_a_hole_between_two_chains_is_not_emitted(ctx):
    assert check(ctx, [(0, 0, "5="), (0, 8, "5=")], "a hole") == [(0, 5, 0, 1, 1, 0), (8, 13, 0, 1, 1, 0)]


# ---- groups and emptiness ----

def test_two_groups_with_equal_positions_and_an_empty_group_between(ctx):
    want = check(ctx, [(0, 50, "10="), (2, 50, "10="), (2, 55, "2X")], "equal positions in two groups", n_groups=4)
    assert want == [(50, 60, 0, 1, 1, 0), (50, 55, 2, 1, 1, 0), (55, 57, 2, 2, 1, 0), (57, 60, 2, 1, 1, 0)]
    segs, seg_first = ctx.cigar_depth(*arrays(["10=", "10=", "2X"])[:2], at_of([(0, 50, 0), (2, 50, 0), (2, 55, 0)]), 4)
    assert seg_first.tolist() == [0, 1, 1, 4, 4]
    assert check(ctx, [(1, 7, "3=")], "n_groups left out: the last chain's group + 1") == [(7, 10, 1, 1, 1, 0)]


def test_empty_chains_and_chains_without_a_reference_base(ctx):
    specs = [(0, 0, ""), (0, 0, "6=2I6="), (0, 3, ""), (0, 4, "3I"), (0, 0, ""), (0, 0, "12="), (1, 7, ""), (1, 0, "3=1I3="), (1, 0, "")]
    assert check(ctx, specs, "empty chains") == [(0, 12, 0, 2, 2, 0), (0, 6, 1, 1, 1, 0)]
    assert check(ctx, [(0, 5, ""), (0, 6, "")], "only empty chains") == []
    assert check(ctx, [(0, 5, "2I"), (1, 6, "1I")], "only insertions: entries, but no event that counts") == []


def test_one_chain_and_no_chain_at_all(ctx):
    assert check(ctx, [(0, 7, "3=2I1X4D2=1I1=")], "one chain") == [(7, 10, 0, 1, 1, 0), (10, 11, 0, 1, 0, 0), (11, 15, 0, 1, 0, 1), (15, 18, 0, 1, 1, 0)]
    before = ctx.timing("cigar_depth_events")[1], ctx.timing("cigar_depth_emit")[1]
    assert before[0] > 0 and before[1] > 0
    segs, seg_first = ctx.cigar_depth(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), 0)
    assert segs.size == 0 and seg_first.tolist() == [0]
    segs, seg_first = ctx.cigar_depth(np.zeros(0, dtype=np.uint64), arrays([])[1], at_of([]), 3)
    assert segs.size == 0 and seg_first.tolist() == [0, 0, 0, 0]
    assert (ctx.timing("cigar_depth_events")[1], ctx.timing("cigar_depth_emit")[1]) == before, "no chain: nothing is launched"


# ---- scale and range ----

def test_600_chains_stacked_on_one_base_range(ctx):
    "a count beyond 255"
    assert check(ctx, [(0, 100, "50=")] * 600, "600 stacked chains") == [(100, 150, 0, 600, 600, 0)]
    want = check(ctx, [(0, 100, "50=")] * 300 + [(0, 120, "10D")] * 300, "300 = and 300 D")
    assert want == [(100, 120, 0, 300, 300, 0), (120, 130, 0, 600, 300, 300), (130, 150, 0, 300, 300, 0)]


def test_one_run_crossed_by_600_other_chains_boundaries(ctx):
    specs = [(0, 1000, "20000=")] + [(0, 1000 + 30 * j, "20X") for j in range(600)]
    want = check(ctx, specs, "600 chains across one run")
    assert len(want) == 1200 and want[0] == (1000, 1020, 0, 2, 1, 0) and want[1] == (1020, 1030, 0, 1, 1, 0) and want[-1] == (18990, 21000, 0, 1, 1, 0)


def test_reference_bases_beyond_2_to_the_32(ctx):
    t0 = (1 << 33) + 5
    assert check(ctx, [(0, t0, "4=1X"), (0, t0 + 2, "4=")], "t0 beyond 2^32") == \
        [(t0, t0 + 2, 0, 1, 1, 0), (t0 + 2, t0 + 4, 0, 2, 2, 0), (t0 + 4, t0 + 5, 0, 2, 1, 0), (t0 + 5, t0 + 6, 0, 1, 1, 0)]


def test_300_random_chains_in_40_groups(ctx):
    want = check(ctx, random_groups(5, 300, 40), "300 random chains", n_groups=40)
    assert len(want) > 300 and max(s[3] for s in want) > 3 and any(s[5] for s in want) and any(s[0] > 1 << 32 for s in want)
    check(ctx, random_groups(6, 300, 40), "300 other random chains", n_groups=40)


# ---- refusals ----

def raw_call(ctx, cigar, recs, at, n_groups, seg_first, n_cigar=None, n_chains=None):
    "the C call itself, with sizes that need not be the arrays': (return code, the segments' pointer as the call left it)"
    p_segs = ctypes.c_void_p()
    rc = ctx.lib.nts_cigar_depth(ctx.h, cigar.ctypes.data, cigar.size if n_cigar is None else n_cigar, recs.ctypes.data,
                                 recs.size if n_chains is None else n_chains, at.ctypes.data, n_groups, ctypes.byref(p_segs), seg_first.ctypes.data)
    return rc, p_segs.value


def refused(ctx, specs, code, words, n_groups=None, mutate=None):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays([s[2] for s in specs])
    if mutate:
        mutate(cigar, recs)
    with pytest.raises(NtsError) as err:
        ctx.cigar_depth(cigar, recs, at_of(specs), n_groups)
    assert f"(code {code})" in str(err.value) and "nts_cigar_depth" in str(err.value) and all(w in str(err.value) for w in words), \
        (code, words, str(err.value))


def test_refusals_name_the_smallest_offending_chain(ctx):
    good = (0, 0, "4=1I4=")
    refused(ctx, [good, (1, 0, "4="), (0, 0, "4="), (0, 0, "1I4=")], EINVAL, ["chain 2", "nondecreasing"], n_groups=2)
    refused(ctx, [good, good, (2, 0, "4="), (3, 0, "4=")], EINVAL, ["chain 2", "n_groups"], n_groups=2)
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | P, 4 << 4 | EQ]), (0, 0, [1 << 4 | EQ, 1 << 4 | P, 1 << 4 | X])], EINVAL, ["chain 1", "code 6"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 2 << 4 | 3, 4 << 4 | EQ]), (0, 0, [2 << 4 | 3])], EINVAL, ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 0, [4 << 4 | EQ, 0 << 4 | D, 4 << 4 | EQ])], EINVAL, ["chain 1", "no CIGAR of its lengths"])
    refused(ctx, [good, (0, 1 << 32, "4="), (0, 1 << 33, "4=")], ERANGE, ["chain 1", "2^32"])
    refused(ctx, [good, (0, (1 << 64) - 2, "4="), (0, (1 << 64) - 1, "4=")], ERANGE, ["chain 1", "wraps"])

    def long(cigar, recs):
        recs["len_a"][1] = 1 << 62
    refused(ctx, [good, (0, 0, "4=")], ERANGE, ["2^62 bases or more"], mutate=long)

    def sums(cigar, recs):
        recs["len_b"][:] = 1 << 61
    refused(ctx, [good, (0, 0, "4=")], ERANGE, ["2^62 bases or more"], mutate=sums)

    def shift(cigar, recs):
        recs["first"][1] += 1
    refused(ctx, [good, (0, 0, "4="), (0, 0, "4=")], EINVAL, ["chain 1", "tile"], mutate=shift)

    def short(cigar, recs):
        recs["len_a"][1] -= 1
    refused(ctx, [good, (0, 0, "4=2D"), (0, 0, "4=")], EINVAL, ["chain 1", "no CIGAR of its lengths"], mutate=short)
    assert check(ctx, [good, (0, (1 << 32) - 9, "4=")], "an extent of 2^32 - 1 - 4 bases passes") == \
        [(0, 8, 0, 1, 1, 0), ((1 << 32) - 9, (1 << 32) - 5, 0, 1, 1, 0)]


def test_2_to_the_32_entries_chains_or_groups_are_refused_before_any_array_is_read(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays(["4="])
    at = at_of([(0, 0, 0)])
    for sizes in (dict(n_cigar=1 << 32), dict(n_chains=1 << 32), dict(n_groups=1 << 32)):
        seg_first = np.full(2, 0xABABABABABABABAB, dtype=np.uint64)
        rc, p_segs = raw_call(ctx, cigar, recs, at, sizes.pop("n_groups", 1), seg_first, **sizes)
        assert rc == ERANGE and p_segs is None and seg_first.tolist() == [0xABABABABABABABAB] * 2, sizes
        with pytest.raises(NtsError) as err:
            ctx.check(rc, "nts_cigar_depth")
        assert "2^32 entries, chains or groups or more" in str(err.value)


def one_entry_chains(n):
    "n chains `1=` of group 0 at base 0, made as arrays"
    from ntsynt_amd.device import CHAIN_DTYPE, CIG_PAD_AT_DTYPE
    recs = np.zeros(n, dtype=CHAIN_DTYPE)
    recs["first"], recs["n_cig"], recs["eq"], recs["len_a"], recs["len_b"] = np.arange(n), 1, 1, 1, 1
    return np.full(n, 1 << 4 | EQ, dtype=np.uint64), recs, np.zeros(n, dtype=CIG_PAD_AT_DTYPE)


def test_a_group_of_2_to_the_20_chains_is_refused_and_one_chain_fewer_is_counted(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, at = one_entry_chains(1 << 20)
    with pytest.raises(NtsError) as err:
        ctx.cigar_depth(cigar, recs, at, 1)
    assert f"(code {ERANGE})" in str(err.value) and f"chain {(1 << 20) - 1}" in str(err.value) and "2^20 chains" in str(err.value)
    at["group"][1 << 19:] = 1                                 # (two groups of 2^19 chains pass)
    segs, seg_first = ctx.cigar_depth(cigar, recs, at, 2)
    assert as_tuples(segs) == [(0, 1, 0, 1 << 19, 1 << 19, 0), (0, 1, 1, 1 << 19, 1 << 19, 0)] and seg_first.tolist() == [0, 1, 2]
    segs, seg_first = ctx.cigar_depth(cigar[:-1], recs[:-1], one_entry_chains((1 << 20) - 1)[2], 1)
    assert as_tuples(segs) == [(0, 1, 0, (1 << 20) - 1, (1 << 20) - 1, 0)] and seg_first.tolist() == [0, 1]


def test_a_refused_call_leaves_seg_first_as_passed_in(ctx):
    for specs, n_groups, code in (([(0, 0, "4="), (0, 0, [4 << 4 | EQ, 2 << 4 | P])], 1, EINVAL),        # behind the first scan
                                  ([(0, 0, "4="), (0, 0, [2 << 4 | 5])], 1, EINVAL),                      # behind the first scan
                                  ([(1, 0, "4="), (0, 0, "4=")], 2, EINVAL),                              # before any launch
                                  ([(0, 0, "4="), (0, 1 << 32, "4=")], 1, ERANGE)):
        cigar, recs, _ = arrays([s[2] for s in specs])
        seg_first = np.full(n_groups + 1, 0xABABABABABABABAB, dtype=np.uint64)
        rc, p_segs = raw_call(ctx, cigar, recs, at_of(specs), n_groups, seg_first)
        assert rc == code and p_segs is None and seg_first.tolist() == [0xABABABABABABABAB] * (n_groups + 1), specs
    assert check(ctx, [(0, 0, "4=")], "the context still answers") == [(0, 4, 0, 1, 1, 0)]

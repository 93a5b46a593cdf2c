"""nts_cigar_lift_stats (csrc/nts_cigar.inc, Context.cigar_lift_stats; docs/design/04_25_lift_identity.md) against
tests/lift_stats_brute.py in every field of every record, on CIGARs and chain records fabricated in NumPy (no genome is read): EVERY
range lo < hi on BOTH sides of small chains with gaps inside and at either end and neighbouring entries of every kind; an empty chain
between two others; the last base of the last chain; an entry of 2^32 + 2 bases (the expectation is a formula in the entry's length,
checked against the brute force at a small length first); one chain of 70 000 entries with lo and hi at entry borders and one base to
either side over spans of 1, 2, 3, 1 000 and all entries; 255, 256, 257 and 513 ranges (workgroup seams); 300 random chains of 2 000
entries with 10 000 random ranges in random order; no range; agreement with nts_cigar_lift on the same input; a small, a four times
larger and again the small case in ONE context with cigar_lift and cigar_build between them; and every refusal, each naming the
smallest offender and leaving `stats` untouched.  Every case's expectation is computed on the CPU before the GPU is called.  Every test
runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import lift_brute as LB
from tests import lift_stats_brute as SB
from tests.test_gpu_cigar_lift import arrays, queries_of, random_chains

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
SMALL = ("5=1X3I2D4=", "3D2I6=", "4=2I", "1=", "3=3=", "2=2D2D1X", "1=2I2I3=")


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


def ranges_of(quads):
    from ntsynt_amd.device import LIFT_RANGE_DTYPE
    return np.array([tuple(q) for q in quads], dtype=LIFT_RANGE_DTYPE) if len(quads) else np.zeros(0, dtype=LIFT_RANGE_DTYPE)


def check(ctx, cigar, recs, quads, want, what):
    from ntsynt_amd.device import LIFT_STATS_DTYPE
    rs = ranges_of(quads)
    got = ctx.cigar_lift_stats(cigar, recs, rs)
    again = ctx.cigar_lift_stats(cigar, recs, rs)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {rs.size} ranges")
    assert got.dtype == LIFT_STATS_DTYPE and got.shape == (len(quads),)
    have = list(zip(*(got[f].tolist() for f in SB.FIELDS))) if got.size else []
    assert have == list(want), (what, [(q, h, w) for q, h, w in zip(quads, have, want) if h != w][:3])
    assert not got["reserved"].any() and got.tobytes() == again.tobytes(), what
    both = got["eq"] + got["x"]
    assert np.array_equal(both + got["src_gap"], rs["hi"] - rs["lo"]) and np.array_equal(both + got["oth_gap"], got["oth_hi"] - got["oth_lo"]), what
    return got


def every_range(recs, lists):
    "every valid range of every chain, both sides, and its brute-force record"
    quads, want = [], []
    for c, entries in enumerate(lists):
        counter = SB.Counter(entries)
        for side in (0, 1):
            n = int(recs[c]["len_b" if side else "len_a"])
            for lo in range(n):
                for hi in range(lo + 1, n + 1):
                    quads.append((c, side, lo, hi))
                    want.append(counter.stats(side, lo, hi))
    return quads, want


def test_every_range_on_both_sides_of_small_chains(ctx):
    for text in SMALL:                                        # each alone (`3=3=`, `2=2D2D1X`, `1=2I2I3=`: neighbouring entries of one kind)
        cigar, recs, lists = arrays([text])
        assert cigar.size == sum(ch in "=XID" for ch in text)
        a, b = int(recs[0]["len_a"]), int(recs[0]["len_b"])
        quads, want = every_range(recs, lists)
        assert len(quads) == a * (a + 1) // 2 + b * (b + 1) // 2
        check(ctx, cigar, recs, quads, want, text)
    cigar, recs, lists = arrays(SMALL)                        # and all in one call
    quads, want = every_range(recs, lists)
    assert {w[6] for w in want} >= {0, 1} and {w[7] for w in want} >= {0, 1} and any(w[0] == w[1] for w in want)
    check(ctx, cigar, recs, quads, want, "the small chains together")
    # what the definition says of gaps, spelled out: `5=1X3I2D4=`, A = 12 bases, B = 13 (tests/test_lift_stats_host.py counts these by hand)
    cigar, recs, _ = arrays(["5=1X3I2D4="])
    check(ctx, cigar, recs, [(0, 0, 7, 9), (0, 0, 4, 7), (0, 0, 0, 6), (0, 1, 7, 10), (0, 1, 6, 9), (0, 0, 0, 12)],
          [(9, 10, 1, 0, 1, 0, 1, 0), (4, 9, 1, 1, 1, 3, 1, 1), (0, 6, 5, 1, 0, 0, 0, 0), (6, 9, 1, 0, 2, 2, 1, 1), (6, 6, 0, 0, 3, 0, 1, 0),
           (0, 13, 9, 1, 2, 3, 1, 1)], "gaps")
    # runs across entries of one kind count once; two runs of one kind count twice
    cigar, recs, lists = arrays(["2=2D2D1X3=1D1D2=2I1=2I1I1="])
    assert (int(recs[0]["len_a"]), int(recs[0]["len_b"])) == (16, 15)
    check(ctx, cigar, recs, [(0, 0, 0, 16), (0, 1, 0, 15)], [SB.range_stats(lists[0], 0, 0, 16), SB.range_stats(lists[0], 1, 0, 15)], "runs")
    assert SB.range_stats(lists[0], 0, 0, 16)[6:] == (2, 2) and SB.range_stats(lists[0], 1, 0, 15)[6:] == (2, 2)


def test_an_empty_chain_between_two_others(ctx):
    cigar, recs, lists = arrays(["2=1D", [], "1I3="])
    assert [int(r["first"]) for r in recs] == [0, 2, 2] and int(recs[1]["n_cig"]) == 0
    quads, want = every_range(recs, lists)
    assert {q[0] for q in quads} == {0, 2}                                                  # (an empty chain has no valid range)
    check(ctx, cigar, recs, quads, want, "an empty chain in the middle")
    check(ctx, *arrays([[], "2=", []])[:2], [(1, 0, 0, 2), (1, 1, 1, 2)], [(0, 2, 2, 0, 0, 0, 0, 0), (1, 2, 1, 0, 0, 0, 0, 0)], "empty chains at both ends")


def test_the_last_base_of_the_last_chain(ctx):
    cigar, recs, lists = arrays(["4=2I", "3D2I6=", "7=1D", "2=3I"])
    quads = [(2, 0, 7, 8), (2, 0, 0, 8), (2, 1, 6, 7), (3, 1, 4, 5), (3, 1, 0, 5), (3, 0, 1, 2), (3, 0, 0, 2)]
    check(ctx, cigar, recs, quads, [SB.range_stats(lists[c], s, lo, hi) for c, s, lo, hi in quads], "the global end")
    got = ctx.cigar_lift_stats(cigar, recs, ranges_of([(3, 1, 4, 5)]))
    assert (int(got[0]["oth_lo"]), int(got[0]["oth_hi"]), int(got[0]["src_gap"])) == (2, 2, 1)


def long_entry_case(big):
    "chains `3=` and `<big>=1I2=`, ranges across the long entry, and the records as formulas in its length"
    chains = [[3 << 4 | EQ], [big << 4 | EQ, 1 << 4 | I, 2 << 4 | EQ]]
    quads = [(1, 0, 0, big + 2), (1, 1, 0, big + 3), (1, 0, big - 1, big + 1), (1, 1, big - 1, big + 1), (1, 0, 1, big), (1, 1, big, big + 1),
             (1, 1, big, big + 3), (1, 0, big - 2, big + 2), (0, 0, 0, 3)]
    want = [(0, big + 3, big + 2, 0, 0, 1, 0, 1), (0, big + 2, big + 2, 0, 1, 0, 1, 0), (big - 1, big + 2, 2, 0, 0, 1, 0, 1), (big - 1, big, 1, 0, 1, 0, 1, 0),
            (1, big, big - 1, 0, 0, 0, 0, 0), (big, big, 0, 0, 1, 0, 1, 0), (big, big + 2, 2, 0, 1, 0, 1, 0), (big - 2, big + 3, 4, 0, 0, 1, 0, 1),
            (0, 3, 3, 0, 0, 0, 0, 0)]
    return chains, quads, want


def test_an_entry_longer_than_32_bits(ctx):
    chains, quads, want = long_entry_case(6)                  # the formulas, against the brute force at a length it can walk
    assert want == [SB.range_stats(chains[c], s, lo, hi) for c, s, lo, hi in quads]
    chains, quads, want = long_entry_case(2 ** 32 + 2)
    cigar, recs, _ = arrays(chains)
    check(ctx, cigar, recs, quads, want, "2^32 + 2")


def test_a_chain_of_70_000_entries_at_entry_borders(ctx):
    rng = np.random.default_rng(5)
    n = 70_000
    codes = np.array([EQ, X, EQ, I, EQ, D, D, EQ, I, I], dtype=np.uint64)[np.arange(n) % 10]
    lens = rng.integers(1, 4, n).astype(np.uint64)
    head, tail = [9 << 4 | EQ], [2 << 4 | D, 4 << 4 | EQ]
    cigar, recs, lists = arrays([head, ((lens << np.uint64(4)) | codes).tolist(), tail])
    counter = SB.Counter(lists[1])
    quads = []
    for side, skip in ((0, I), (1, D)):
        consumed = np.where(codes != skip, lens, 0).astype(np.int64)
        border = np.concatenate([[0], np.cumsum(consumed)])   # the source bases in front of every entry
        total = int(border[-1])
        for span, starts in ((1, 40), (2, 40), (3, 40), (1000, 12), (n, 1)):
            for e in np.linspace(0, n - span, starts).astype(np.int64).tolist():
                for lo in (border[e] - 1, border[e], border[e] + 1):
                    for hi in (border[e + span] - 1, border[e + span], border[e + span] + 1):
                        if 0 <= lo < hi <= total:
                            quads.append((1, side, int(lo), int(hi)))
    want = [counter.stats(side, lo, hi) for _, side, lo, hi in quads]
    assert len(quads) > 1500 and max(w[6] for w in want) > 10_000 and max(w[7] for w in want) > 10_000
    check(ctx, cigar, recs, quads, want, "70 000 entries")


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_workgroup_seams(ctx, n):
    cigar, recs, lists = arrays(["5=1X3I2D4=", "3D2I6=", "4=2I"])
    every, stats = every_range(recs, lists)
    pick = [(7 * q) % len(every) for q in range(n)]
    check(ctx, cigar, recs, [every[p] for p in pick], [stats[p] for p in pick], f"{n} ranges")


def random_ranges(rng, recs, count):
    quads = []
    while len(quads) < count:
        c, side = int(rng.integers(0, recs.size)), int(rng.integers(0, 2))
        n = int(recs[c]["len_b" if side else "len_a"])
        lo, hi = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        if lo < hi:
            quads.append((c, side, lo, hi if rng.integers(0, 4) else min(lo + int(rng.integers(1, 8)), n)))
    return quads


def test_random_chains_and_ranges(ctx):
    cigar, recs, lists = arrays(random_chains(11))
    quads = random_ranges(np.random.default_rng(12), recs, 10_000)
    counters, want = {}, []
    for c, side, lo, hi in quads:
        if c not in counters:
            counters[c] = SB.Counter(lists[c])
        want.append(counters[c].stats(side, lo, hi))
    assert len(counters) > 250 and any(w[2] + w[3] + w[4] + w[5] < 4 for w in want) and max(w[6] for w in want) > 100
    check(ctx, cigar, recs, quads, want, "300 random chains")


def test_no_range(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays(["4=2I", "1="])
    scans, searches = ctx.timing("lift_stats_scan")[1], ctx.timing("lift_stats_search")[1]
    got = check(ctx, cigar, recs, [], [], "no range")
    assert got.size == 0 and ctx.timing("lift_stats_search")[1] == searches and ctx.timing("lift_stats_scan")[1] > scans        # (pass 1 ran, no search)
    check(ctx, np.zeros(0, dtype=np.uint64), recs[:0], [], [], "nothing at all")
    bad = cigar.copy()
    bad[0] = 4 << 4 | 3
    with pytest.raises(NtsError, match="entries of chain 0"):                               # (the entries are still checked)
        ctx.cigar_lift_stats(bad, recs, ranges_of([]))


def test_agreement_with_cigar_lift_on_the_same_input(ctx):
    cigar, recs, _ = arrays(random_chains(13, 20, 300))
    quads = random_ranges(np.random.default_rng(14), recs, 4000)
    rs = ranges_of(quads)
    hits = ctx.cigar_lift(cigar, recs, queries_of([t for c, side, lo, hi in quads for t in ((c, side, lo), (c, side, hi - 1))]))
    stats = ctx.cigar_lift_stats(cigar, recs, rs)
    left, right = hits[0::2], hits[1::2]
    assert np.array_equal(stats["oth_lo"], left["pos"])
    assert np.array_equal(stats["oth_hi"], right["pos"] + np.isin(right["code"], (EQ, X)))
    assert np.array_equal(stats["eq"] + stats["x"] + stats["src_gap"], rs["hi"] - rs["lo"])
    assert np.array_equal(stats["eq"] + stats["x"] + stats["oth_gap"], stats["oth_hi"] - stats["oth_lo"])
    assert len({int(c) for c in right["code"]}) >= 3 and np.any(stats["oth_lo"] == stats["oth_hi"])


def test_small_large_small_in_one_context_between_other_calls():
    "docs/design/04_24_call_order.md: a pointer from ws_get is dead after a later request of its name -- L regrows every buffer S made"
    from ntsynt_amd.device import Context
    cases = {}
    for size, (n_chains, n_entries, n_ranges) in (("S", (6, 30, 48)), ("L", (30, 150, 240))):
        cigar, recs, lists = arrays(random_chains(31 if size == "S" else 32, n_chains, n_entries))
        quads = random_ranges(np.random.default_rng(33), recs, n_ranges)
        counters = [SB.Counter(entries) for entries in lists]
        cases[size] = (cigar, recs, quads, [counters[c].stats(side, lo, hi) for c, side, lo, hi in quads])
    assert all(len(cases["L"][i]) >= 4 * len(cases["S"][i]) for i in range(3))
    others = {(name, size): (C.case_of(name, size), C.expected_of(name, size)) for name in ("cigar_build", "cigar_lift") for size in C.SIZES}
    ctx = Context(0)
    try:
        for step, size in enumerate(("S", "L", "S", "L", "S")):
            check(ctx, *cases[size], f"step {step}, {size}")
            for name in ("cigar_lift", "cigar_build"):        # (sizes that rise and fall between the calls under test)
                other = "L" if step % 2 == 0 else "S"
                assert C.BY_NAME[name].run(ctx, others[(name, other)][0]) == others[(name, other)][1], (step, name, other)
    finally:
        ctx.close()


def refused(ctx, cigar, recs, quads, code, *words, counts=None, null=False):
    "the call through the library itself: the return code, the message, `stats` untouched.  counts: (n_cigar, n_chains, n_ranges) other than the arrays'"
    from ntsynt_amd.device import LIFT_STATS_DTYPE
    rs = ranges_of(quads)
    stats = np.full(max(rs.size, 1) * LIFT_STATS_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    before = stats.tobytes()
    n = counts or (cigar.size, recs.size, rs.size)
    pointers = (None, None, None, None) if null else (cigar.ctypes.data, recs.ctypes.data, rs.ctypes.data, stats.ctypes.data)
    rc = ctx.lib.nts_cigar_lift_stats(ctx.h, pointers[0], int(n[0]), pointers[1], int(n[1]), pointers[2], int(n[2]), pointers[3])
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert stats.tobytes() == before
    return said


def test_ranges_outside_their_chain_are_refused(ctx):
    cigar, recs, _ = arrays(["5=1X3I2D4=", "3D2I6="])
    good = [(0, 0, 3, 9), (1, 1, 0, 8), (0, 1, 12, 13), (1, 0, 8, 9)] * 70                   # (more than one workgroup)
    for bad, at in (((0, 0, 4, 4), 5), ((0, 0, 5, 4), 17), ((0, 0, 3, 13), 256), ((1, 1, 0, 9), 0), ((2, 0, 0, 1), 100), ((0xFFFFFFFF, 0, 0, 1), 279),
                    ((0, 2, 0, 1), 3), ((0, 0, 12, 13), 8), ((0, 0, 0, 2 ** 63), 31), ((0, 0, 2 ** 64 - 1, 0), 2)):
        quads = list(good)
        quads[at] = bad
        quads[-1] = (1, 0, 3, 10)                                                           # (a later offender as well: the smallest one is named)
        refused(ctx, cigar, recs, quads, -22, f"nts_cigar_lift_stats: range {at} is outside its chain")
    from ntsynt_amd.device import NtsError
    with pytest.raises(NtsError, match="range 1 is outside its chain"):
        ctx.cigar_lift_stats(cigar, recs, ranges_of([(0, 0, 0, 1), (0, 0, 6, 6)]))
    empty, empty_recs, _ = arrays(["2=", []])
    refused(ctx, empty, empty_recs, [(0, 0, 0, 2), (1, 0, 0, 1)], -22, "range 1 is outside its chain")    # (an empty chain holds no base)


def test_entries_that_are_no_cigar_are_refused(ctx):
    cigar, recs, _ = arrays(["2=", "5=1X3I2D4=", "3D2I6=", "4="])
    some = [(1, 0, 3, 9), (2, 1, 1, 2)]
    assert cigar.size == 10 and [int(r["first"]) for r in recs] == [0, 1, 6, 9]
    for at, value, chain in ((3, 1 << 4 | 3, 1), (7, 2 << 4 | 0, 2), (4, 0 << 4 | I, 1), (0, 0 << 4 | EQ, 0), (9, 7 << 4 | 15, 3)):
        bad = cigar.copy()
        bad[9] = 7 << 4 | 15                                  # (a later offender as well: the smallest chain is named)
        bad[at] = value
        refused(ctx, bad, recs, some, -22, f"nts_cigar_lift_stats: the entries of chain {chain} are no CIGAR of its lengths")
    for field in ("len_a", "len_b"):
        for delta in (1, -1):
            off = recs.copy()
            off[field][2] = int(off[field][2]) + delta
            off["len_a"][3] += 1
            refused(ctx, cigar, off, some, -22, "the entries of chain 2 are no CIGAR of its lengths")
    # a range outside its chain as well: the CIGAR is named first
    refused(ctx, np.where(np.arange(cigar.size) == 3, 1 << 4 | 3, cigar).astype(np.uint64), recs, [(9, 0, 0, 1)], -22, "the entries of chain 1")


def test_refusals_before_any_launch(ctx):
    cigar, recs, _ = arrays(["2=", "5=1X3I2D4=", "3D2I6="])
    some = [(1, 0, 3, 4)]
    scans = ctx.timing("lift_stats_scan")[1]
    beyond = recs.copy()
    beyond["n_cig"][1] += 4                                                                  # 1 + 5 + 4 = 10 > 9 entries
    beyond["n_cig"][2] += 1
    refused(ctx, cigar, beyond, some, -22, "nts_cigar_lift_stats: chain 1", "beyond n_cigar")
    beyond = recs.copy()
    beyond["first"][2] = 2 ** 64 - 1                                                         # (first + n_cig wraps)
    refused(ctx, cigar, beyond, some, -22, "chain 2", "beyond n_cigar")
    back = recs.copy()
    back["first"][2] = 0
    refused(ctx, cigar, back, some, -22, "chain 2", "nondecreasing")
    for counts in ((2 ** 32, 3, 1), (9, 2 ** 32, 1), (9, 3, 2 ** 32)):                       # refused before any array is read: null pointers
        refused(ctx, cigar, recs, some, -34, "2^32", counts=counts, null=True)
    huge = recs.copy()
    huge["len_a"][0], huge["len_a"][1] = 2 ** 62, 2 ** 62                                    # together 2^63
    refused(ctx, cigar, huge, some, -34, "2^63")
    huge = recs.copy()
    huge["len_b"][2] = 2 ** 64 - 1
    refused(ctx, cigar, huge, some, -34, "2^63")
    assert ctx.timing("lift_stats_scan")[1] == scans

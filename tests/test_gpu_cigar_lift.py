"""nts_cigar_lift (csrc/nts_cigar.inc, Context.cigar_lift; docs/design/04_23_block_lift.md) against tests/lift_brute.py in every field of
every hit, on CIGARs and chain records fabricated in NumPy (no genome is read): EVERY position 0 .. len on BOTH sides of small chains
with gaps inside and at either end, one entry, and two neighbouring entries of one kind; an empty chain between two others; the last
position of the last chain (the global end of the prefixes); an entry of 2^32 + 2 bases; one chain of 70 000 entries queried at every
entry border and one base to either side (searches of 17 steps, prefixes across scan tiles); 255, 256, 257 and 513 queries (workgroup
seams); 300 random chains of 2 000 entries with 10 000 random queries in random order; no query; there and back again; and every
refusal, each naming the smallest offender and leaving `hits` untouched.  Every case's expectation is computed on the CPU before the
GPU is called.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import lift_brute as LB

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
SMALL = ("5=1X3I2D4=", "3D2I6=", "4=2I", "1=", "3=3=")


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


def arrays(chains):
    "chains: per chain its entries (a CIGAR string or a list of len << 4 | code).  Returns (cigar, CHAIN array, the entry lists)"
    from ntsynt_amd.device import CHAIN_DTYPE
    lists = [LB.parse_cigar(c) if isinstance(c, str) else list(c) for c in chains]
    recs = np.zeros(len(lists), dtype=CHAIN_DTYPE)
    at = 0
    for c, entries in enumerate(lists):
        count = {code: sum(v >> 4 for v in entries if v & 15 == code) for code in (I, D, EQ, X)}
        recs[c] = (at, len(entries), count[EQ], count[X], count[I], count[D], count[EQ] + count[X] + count[D], count[EQ] + count[X] + count[I])
        at += len(entries)
    return np.array([v for entries in lists for v in entries], dtype=np.uint64), recs, lists


def queries_of(triples):
    from ntsynt_amd.device import LIFT_QUERY_DTYPE
    return np.array([tuple(t) for t in triples], dtype=LIFT_QUERY_DTYPE) if len(triples) else np.zeros(0, dtype=LIFT_QUERY_DTYPE)


def check(ctx, cigar, recs, triples, want, what):
    from ntsynt_amd.device import LIFT_HIT_DTYPE
    qs = queries_of(triples)
    got = ctx.cigar_lift(cigar, recs, qs)
    again = ctx.cigar_lift(cigar, recs, qs)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {qs.size} queries")
    assert got.dtype == LIFT_HIT_DTYPE and got.shape == (len(triples),)
    have = [(int(h["pos"]), int(h["entry"]), int(h["off"]), int(h["code"])) for h in got]
    assert have == list(want), (what, [(t, h, w) for t, h, w in zip(triples, have, want) if h != w][:3])
    assert not got["reserved"].any() and got.tobytes() == again.tobytes(), what
    return got


def every_position(recs, lists):
    "every valid query of every chain, both sides, and its brute-force hit"
    triples, want = [], []
    for c, entries in enumerate(lists):
        for side in (0, 1):
            for pos in range(int(recs[c]["len_b" if side else "len_a"]) + 1):
                triples.append((c, side, pos))
                want.append(LB.lift(entries, side, pos, int(recs[c]["first"])))
    return triples, want


def test_every_position_on_both_sides_of_small_chains(ctx):
    for text in SMALL:                                        # each alone (`3=3=`: two entries of one kind, as parse_cigar leaves them)
        cigar, recs, lists = arrays([text])
        assert cigar.size == sum(ch in "=XID" for ch in text)
        triples, want = every_position(recs, lists)
        assert len(triples) == int(recs[0]["len_a"]) + int(recs[0]["len_b"]) + 2
        check(ctx, cigar, recs, triples, want, text)
    cigar, recs, lists = arrays(SMALL)                                # and all in one call
    triples, want = every_position(recs, lists)
    check(ctx, cigar, recs, triples, want, "the small chains together")
    # what the definition says of gaps, spelled out: `5=1X3I2D4=`, A = 12 bases, B = 13
    cigar, recs, _ = arrays(["5=1X3I2D4="])
    check(ctx, cigar, recs, [(0, 0, 5), (0, 0, 6), (0, 0, 7), (0, 0, 8), (0, 1, 6), (0, 1, 8), (0, 1, 9), (0, 0, 12), (0, 1, 13)],
          [(5, 1, 0, X), (9, 3, 0, D), (9, 3, 1, D), (9, 4, 0, EQ), (6, 2, 0, I), (6, 2, 2, I), (8, 4, 0, EQ), (13, 5, 0, 0), (12, 5, 0, 0)], "gaps")


def test_an_empty_chain_between_two_others(ctx):
    cigar, recs, lists = arrays(["2=1D", [], "1I3="])
    assert [int(r["first"]) for r in recs] == [0, 2, 2] and int(recs[1]["n_cig"]) == 0
    triples, want = every_position(recs, lists)
    assert ((1, 0, 0) in triples) and want[triples.index((1, 0, 0))] == (0, 2, 0, 0) and want[triples.index((1, 1, 0))] == (0, 2, 0, 0)
    check(ctx, cigar, recs, triples, want, "an empty chain in the middle")
    check(ctx, *arrays([[], "2=", []])[:2], [(0, 0, 0), (2, 1, 0), (1, 0, 1)], [(0, 0, 0, 0), (0, 1, 0, 0), (1, 0, 1, EQ)], "empty chains at both ends")


def test_the_last_position_of_the_last_chain(ctx):
    cigar, recs, lists = arrays(["4=2I", "3D2I6=", "7=1D"])
    last = len(lists) - 1
    check(ctx, cigar, recs, [(last, 0, 7), (last, 0, 8), (last, 1, 6), (last, 1, 7)],
          [LB.lift(lists[last], s, p, int(recs[last]["first"])) for s, p in ((0, 7), (0, 8), (1, 6), (1, 7))], "the global end")
    got = ctx.cigar_lift(cigar, recs, queries_of([(last, 0, 8)]))
    assert (int(got[0]["pos"]), int(got[0]["entry"])) == (7, cigar.size)


def test_an_entry_longer_than_32_bits(ctx):
    big = 2 ** 32 + 2
    cigar, recs, _ = arrays([[3 << 4 | EQ], [big << 4 | EQ, 1 << 4 | I, 2 << 4 | EQ]])
    check(ctx, cigar, recs, [(1, 0, big - 1), (1, 1, big - 1), (1, 0, big), (1, 1, big), (1, 1, big + 1), (1, 0, big + 2), (1, 1, big + 3), (0, 0, 2)],
          [(big - 1, 1, big - 1, EQ), (big - 1, 1, big - 1, EQ), (big + 1, 3, 0, EQ), (big, 2, 0, I), (big, 3, 0, EQ), (big + 3, 4, 0, 0), (big + 2, 4, 0, 0),
           (2, 0, 2, EQ)], "2^32 + 2")


def test_a_chain_of_70_000_entries_at_every_entry_border(ctx):
    rng = np.random.default_rng(5)
    codes = np.array([EQ, X, EQ, I, EQ, D], dtype=np.uint64)[np.arange(70_000) % 6]
    lens = rng.integers(1, 4, 70_000).astype(np.uint64)
    head, tail = [9 << 4 | EQ], [2 << 4 | D, 4 << 4 | EQ]
    cigar, recs, lists = arrays([head, ((lens << np.uint64(4)) | codes).tolist(), tail])
    walker = LB.Walker(lists[1], int(recs[1]["first"]))
    triples = []
    for side, skip in ((0, I), (1, D)):
        consumed = np.where(codes != skip, lens, 0).astype(np.int64)
        border = np.concatenate([[0], np.cumsum(consumed)])
        near = np.unique(np.concatenate([border - 1, border, border + 1]))
        triples += [(1, side, int(p)) for p in near if 0 <= p <= border[-1]]
    want = [walker.lift(side, pos) for _, side, pos in triples]
    assert len(triples) > 150_000
    check(ctx, cigar, recs, triples, want, "70 000 entries")


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_workgroup_seams(ctx, n):
    cigar, recs, lists = arrays(["5=1X3I2D4=", "3D2I6=", "4=2I"])
    every, hits = every_position(recs, lists)
    pick = [(7 * q) % len(every) for q in range(n)]
    check(ctx, cigar, recs, [every[p] for p in pick], [hits[p] for p in pick], f"{n} queries")


def random_chains(seed, n_chains=300, n_entries=2000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_chains):
        codes = np.array([EQ, X, I, D])[rng.integers(0, 4, n_entries)]          # (neighbours of one kind are legal input)
        lens = rng.integers(1, 4, n_entries)
        out.append(((lens << 4) | codes).tolist())
    return out


def test_random_chains_and_queries(ctx):
    cigar, recs, lists = arrays(random_chains(11))
    rng = np.random.default_rng(12)
    walkers = {}
    triples = []
    for _ in range(10_000):
        c, side = int(rng.integers(0, len(lists))), int(rng.integers(0, 2))
        triples.append((c, side, int(rng.integers(0, int(recs[c]["len_b" if side else "len_a"]) + 1))))
    want = []
    for c, side, pos in triples:
        if c not in walkers:
            walkers[c] = LB.Walker(lists[c], int(recs[c]["first"]))
        want.append(walkers[c].lift(side, pos))
    assert len(walkers) > 250 and len({h[3] for h in want}) >= 4
    check(ctx, cigar, recs, triples, want, "300 random chains")


def test_no_query(ctx):
    from ntsynt_amd.device import NtsError
    cigar, recs, _ = arrays(["4=2I", "1="])
    searches = ctx.timing("lift_search")[1]
    got = check(ctx, cigar, recs, [], [], "no query")
    assert got.size == 0 and ctx.timing("lift_search")[1] == searches                      # (no search was launched)
    check(ctx, np.zeros(0, dtype=np.uint64), recs[:0], [], [], "nothing at all")
    bad = cigar.copy()
    bad[0] = 4 << 4 | 3
    with pytest.raises(NtsError, match="entries of chain 0"):                               # (the entries are still checked)
        ctx.cigar_lift(bad, recs, queries_of([]))


def test_there_and_back_again(ctx):
    cigar, recs, lists = arrays(random_chains(13, 20, 300))
    triples, want = every_position(recs, lists)
    aligned = [(t, h) for t, h in zip(triples, want) if t[1] == 0 and h[3] in (EQ, X)]
    assert len(aligned) > 5000
    there = ctx.cigar_lift(cigar, recs, queries_of([t for t, _ in aligned]))
    back = ctx.cigar_lift(cigar, recs, queries_of([(t[0], 1, int(h["pos"])) for (t, _), h in zip(aligned, there)]))
    assert back["pos"].tolist() == [t[2] for t, _ in aligned]
    assert back["entry"].tolist() == there["entry"].tolist() and back["off"].tolist() == there["off"].tolist()


def refused(ctx, cigar, recs, triples, code, *words, counts=None):
    "the call through the library itself: the return code, the message, `hits` untouched.  counts: (n_cigar, n_chains, n_queries) other than the arrays'"
    from ntsynt_amd.device import LIFT_HIT_DTYPE
    qs = queries_of(triples)
    hits = np.full(max(qs.size, 1) * LIFT_HIT_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    before = hits.tobytes()
    n = counts or (cigar.size, recs.size, qs.size)
    rc = ctx.lib.nts_cigar_lift(ctx.h, cigar.ctypes.data, int(n[0]), recs.ctypes.data, int(n[1]), qs.ctypes.data, int(n[2]), hits.ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert hits.tobytes() == before
    return said


def test_queries_outside_their_chain_are_refused(ctx):
    cigar, recs, _ = arrays(["5=1X3I2D4=", "3D2I6="])
    good = [(0, 0, 3), (1, 1, 8), (0, 1, 13), (1, 0, 9)] * 70                               # (more than one workgroup)
    for bad, at in (((2, 0, 0), 5), ((0, 2, 0), 17), ((0, 0, 13), 256), ((1, 1, 9), 0), ((0xFFFFFFFF, 0, 0), 279), ((0, 0, 2 ** 63), 3)):
        triples = list(good)
        triples[at] = bad
        triples[-1] = (1, 0, 10)                                                            # (a later offender as well: the smallest one is named)
        refused(ctx, cigar, recs, triples, -22, f"query {at} is outside its chain")
    from ntsynt_amd.device import NtsError
    with pytest.raises(NtsError, match="query 1 is outside its chain"):
        ctx.cigar_lift(cigar, recs, queries_of([(0, 0, 0), (0, 0, 13)]))


def test_entries_that_are_no_cigar_are_refused(ctx):
    cigar, recs, _ = arrays(["2=", "5=1X3I2D4=", "3D2I6=", "4="])
    some = [(1, 0, 3), (2, 1, 1)]
    assert cigar.size == 10 and [int(r["first"]) for r in recs] == [0, 1, 6, 9]
    for at, value, chain in ((3, 1 << 4 | 3, 1), (7, 2 << 4 | 0, 2), (4, 0 << 4 | I, 1), (0, 0 << 4 | EQ, 0), (9, 7 << 4 | 15, 3)):
        bad = cigar.copy()
        bad[9] = 7 << 4 | 15                                  # (a later offender as well: the smallest chain is named)
        bad[at] = value
        refused(ctx, bad, recs, some, -22, f"the entries of chain {chain} are no CIGAR of its lengths")
    for field in ("len_a", "len_b"):
        for delta in (1, -1):
            off = recs.copy()
            off[field][2] = int(off[field][2]) + delta
            off["len_a"][3] += 1
            refused(ctx, cigar, off, some, -22, "the entries of chain 2 are no CIGAR of its lengths")
    # a query outside its chain as well: the CIGAR is named first
    refused(ctx, np.where(np.arange(cigar.size) == 3, 1 << 4 | 3, cigar).astype(np.uint64), recs, [(9, 0, 0)], -22, "the entries of chain 1")


def test_refusals_before_any_launch(ctx):
    cigar, recs, _ = arrays(["2=", "5=1X3I2D4=", "3D2I6="])
    some = [(1, 0, 3)]
    scans = ctx.timing("lift_scan")[1]
    beyond = recs.copy()
    beyond["n_cig"][1] += 4                                                                  # 1 + 5 + 4 = 10 > 9 entries
    beyond["n_cig"][2] += 1
    refused(ctx, cigar, beyond, some, -22, "chain 1", "beyond n_cigar")
    beyond = recs.copy()
    beyond["first"][2] = 2 ** 64 - 1                                                         # (first + n_cig wraps)
    refused(ctx, cigar, beyond, some, -22, "chain 2", "beyond n_cigar")
    back = recs.copy()
    back["first"][2] = 0
    refused(ctx, cigar, back, some, -22, "chain 2", "nondecreasing")
    for counts in ((2 ** 32, 3, 1), (9, 2 ** 32, 1), (9, 3, 2 ** 32)):                       # refused before any array is read
        refused(ctx, cigar, recs, some, -34, "2^32", counts=counts)
    huge = recs.copy()
    huge["len_a"][0], huge["len_a"][1] = 2 ** 62, 2 ** 62                                    # together 2^63
    refused(ctx, cigar, huge, some, -34, "2^63")
    huge = recs.copy()
    huge["len_b"][2] = 2 ** 64 - 1
    refused(ctx, cigar, huge, some, -34, "2^63")
    assert ctx.timing("lift_scan")[1] == scans

"""nts_cigar_lift_pairs (csrc/nts_cigar.inc, Context.cigar_lift_pairs; docs/design/04_27_lift_joined.md) against
tests/lift_pairs_brute.py in every field of every record, on CIGARs, chain records and links fabricated in NumPy (no genome is read):
EVERY range lo < hi over the hull of pairs of 1, 2 and 3 small chains plus 3 bases to either side, on BOTH sides, with open stretches of
0 and of a few bases (a range in an open stretch only, ranges that end at chain borders, chains that begin or end with a gap of their
array neighbour's kind, middle chains counted whole, a chain without a base of one side); one-link pairs against Context.cigar_lift_stats;
chain records shuffled against link order; a pair of 1 000 one-entry chains with lo and hi at every chain border and one base to either
side; 255, 256, 257 and 513 ranges and 257 links; an entry of 2^32 + 2 bases inside a middle chain (the expectation is a formula in
the entry's length, checked against the brute force at a small length first); 300 random pairs of 1 to 6 chains with 10 000 random
ranges in random order; no range; a small, a four times larger and again the small case in ONE context; and every refusal, each naming
the smallest offender and leaving `stats` untouched.  Every case's expectation is computed on the CPU before the GPU is called.  Every
test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import lift_pairs_brute as PB
from tests.test_gpu_cigar_lift import arrays, random_chains

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
# per pair [(chain, open A bases in front of it, open B bases in front of it)]; in front of the first chain: where the pair's first chain starts
SMALL_PAIRS = (
    [("5=1X3I2D4=", 4, 2)],
    [("4=2I", 3, 3), ("3D2I6=", 0, 0)],                       # no open stretch at all
    [("4=2I", 5, 0), ("2I3=", 0, 0), ("2=2D", 2, 0), ("2D2D1X", 0, 3)],                     # I behind I and D behind D across chains: four runs
    [("3D2I6=", 3, 4), ("2=2D2D1X", 3, 0), ("4=2I", 0, 2)],                                 # a middle chain, stretches on one side each
    [("1=", 7, 3), ("5=1X3I2D4=", 2, 5), ("1X", 4, 1)],
    [("3=", 3, 3), ("2I", 1, 1), ("3=", 2, 0)],                                            # the middle chain holds no A base
    [("2D", 3, 3), ("4=", 0, 1), ("1D", 1, 0)],                                            # the end chains hold no B base
)


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


def world(pairs, shuffle=None):
    """pairs as SMALL_PAIRS (a chain is a CIGAR string or a list of entries).  Returns (cigar, records, links, pair_first, walkers): the
    records in link order, or with shuffle (a seed) in a random order; walkers[p] = the brute force of pair p"""
    from ntsynt_amd.device import LIFT_LINK_DTYPE
    from tests import lift_brute as LB
    flat = [LB.parse_cigar(c) if isinstance(c, str) else list(c) for pair in pairs for c, _, _ in pair]
    order = np.arange(len(flat)) if shuffle is None else np.random.default_rng(shuffle).permutation(len(flat))
    cigar, recs, _ = arrays([flat[i] for i in order.tolist()])
    record_of = np.empty(len(flat), dtype=np.int64)
    record_of[order] = np.arange(len(flat))
    links = np.zeros(len(flat), dtype=LIFT_LINK_DTYPE)
    pair_first, walkers, n = [0], [], 0
    for pair in pairs:
        a = b = 0
        placed = []
        for _, da, db in pair:
            rec = recs[record_of[n]]
            a, b = a + da, b + db
            links[n] = (record_of[n], 0, a, b)
            placed.append((flat[n], a, b))
            a, b, n = a + int(rec["len_a"]), b + int(rec["len_b"]), n + 1
        walkers.append(PB.PairWalker(placed, pair_first[-1]) if sum(v >> 4 for e, _, _ in placed for v in e) < 200_000 else None)
        pair_first.append(n)
    return cigar, recs, links, np.array(pair_first, dtype=np.uint64), walkers


def ranges_of(quads):
    from ntsynt_amd.device import PAIR_RANGE_DTYPE
    return np.array([tuple(q) for q in quads], dtype=PAIR_RANGE_DTYPE) if len(quads) else np.zeros(0, dtype=PAIR_RANGE_DTYPE)


def check(ctx, w, quads, want, what):
    from ntsynt_amd.device import PAIR_STATS_DTYPE
    cigar, recs, links, pair_first = w[:4]
    rs = ranges_of(quads)
    got = ctx.cigar_lift_pairs(cigar, recs, links, pair_first, rs)
    again = ctx.cigar_lift_pairs(cigar, recs, links, pair_first, rs)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {links.size} links, {pair_first.size - 1} pairs, {rs.size} ranges")
    assert got.dtype == PAIR_STATS_DTYPE and got.shape == (len(quads),)
    have = list(zip(*(got[f].tolist() for f in PB.FIELDS))) if got.size else []
    assert have == list(want), (what, [(q, h, x) for q, h, x in zip(quads, have, want) if h != x][:3])
    assert not got["reserved"].any() and not got["reserved2"].any() and got.tobytes() == again.tobytes(), what
    both = got["eq"] + got["x"]
    assert np.array_equal(both + got["src_gap"] + got["src_open"], got["src_hi"] - got["src_lo"]), what
    assert np.array_equal(both + got["oth_gap"] + got["oth_open"], got["oth_hi"] - got["oth_lo"]), what
    return got


def hull(walker, side):
    spans = walker.spans
    return (spans[0][2], spans[-1][3]) if side else (spans[0][0], spans[-1][1])


def every_range(walkers, margin=3):
    "every lo < hi over every pair's hull and `margin` bases to either side, both sides, and its brute-force record"
    quads, want = [], []
    for p, walker in enumerate(walkers):
        for side in (0, 1):
            first, last = hull(walker, side)
            for lo in range(max(first - margin, 0), last + margin):
                for hi in range(lo + 1, last + margin + 1):
                    quads.append((p, side, lo, hi))
                    want.append(walker.stats(side, lo, hi))
    return quads, want


def test_every_range_over_small_pairs_on_both_sides(ctx):
    w = world(SMALL_PAIRS)
    quads, want = every_range(w[4])
    assert len(quads) > 3000 and all(PB.identities_hold(x) for x in want)
    assert {x[14] for x in want} == {0, 1, 2, 3, 4} and any(x[8] > 0 and x[9] == 0 for x in want) and any(x[9] > 0 and x[8] == 0 for x in want)
    check(ctx, w, quads, want, "the small pairs together")
    for p in (0, 2, 3):                                       # and some alone: the link prefixes start at 0
        alone = world([SMALL_PAIRS[p]])
        check(ctx, alone, *every_range(alone[4]), f"pair {p} alone")
    # what the definition says, spelled out by hand.  Pair 1: `4=2I` at A 3..7, B 3..9, then `3D2I6=` at A 7..16, B 9..17, no stretch
    by_hand = {(1, 0, 0, 19): (3, 16, 3, 17, 10, 0, 3, 4, 0, 0, 1, 2, 1, 2, 2),
               (1, 0, 6, 8): (6, 8, 6, 9, 1, 0, 1, 2, 0, 0, 1, 1, 1, 2, 2),
               (1, 1, 8, 10): (8, 10, 7, 10, 0, 0, 2, 3, 0, 0, 2, 1, 1, 2, 2),
               # pair 2, A 5..9, 9..12, 14..18, 18..23 and B 0..6, 6..11, 11..13, 16..17: I behind I across chains is two runs, `2D2D` one
               (2, 0, 2, 26): (5, 23, 0, 17, 9, 1, 6, 4, 2, 3, 2, 2, 3, 6, 4),
               # pair 3, A 3..12, 15..22, 22..26 and B 4..12, 12..15, 17..23: the stretch between its first two chains alone; across the middle chain
               (3, 0, 12, 15): PB.NONE,
               (3, 0, 10, 24): (10, 24, 10, 19, 6, 1, 4, 0, 3, 2, 1, 0, 7, 9, 3)}
    for q, record in by_hand.items():
        assert want[quads.index(q)] == record, (q, want[quads.index(q)])


def test_one_link_pairs_equal_cigar_lift_stats(ctx):
    "the existing call is the yardstick: a pair of one chain at (a0, b0) answers as the chain does, moved by a0 and b0"
    chains = random_chains(41, 40, 60)
    rng = np.random.default_rng(42)
    w = world([[(c, int(rng.integers(0, 50)), int(rng.integers(0, 50)))] for c in chains], shuffle=43)
    cigar, recs, links, pair_first, _ = w
    from ntsynt_amd.device import LIFT_RANGE_DTYPE
    quads, local = [], []
    for _ in range(4000):
        p, side = int(rng.integers(0, len(chains))), int(rng.integers(0, 2))
        c = int(links[p]["chain"])
        n, s0 = int(recs[c]["len_b" if side else "len_a"]), int(links[p]["b0" if side else "a0"])
        lo, hi = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        if lo < hi:
            quads.append((p, side, s0 + lo, s0 + hi))
            local.append((c, side, lo, hi))
    per_chain = ctx.cigar_lift_stats(cigar, recs, np.array(local, dtype=LIFT_RANGE_DTYPE))
    got = ctx.cigar_lift_pairs(cigar, recs, links, pair_first, ranges_of(quads))
    q = ranges_of(quads)
    o0 = np.where(q["side"] == 1, links["a0"][q["pair"]], links["b0"][q["pair"]])
    assert np.array_equal(got["src_lo"], q["lo"]) and np.array_equal(got["src_hi"], q["hi"])
    assert np.array_equal(got["oth_lo"], per_chain["oth_lo"] + o0) and np.array_equal(got["oth_hi"], per_chain["oth_hi"] + o0)
    for f in ("eq", "x", "src_gap", "oth_gap", "src_gaps", "oth_gaps"):
        assert np.array_equal(got[f], per_chain[f]), f
    assert not got["src_open"].any() and not got["oth_open"].any() and np.all(got["n_links"] == 1)
    assert np.array_equal(got["link_lo"], q["pair"]) and np.array_equal(got["link_hi"], q["pair"])


def test_chain_records_shuffled_against_link_order(ctx):
    for seed in (1, 2):
        w = world(SMALL_PAIRS, shuffle=seed)
        assert not np.array_equal(w[2]["chain"], np.arange(w[2].size))
        check(ctx, w, *every_range(w[4], margin=1), f"shuffled records, seed {seed}")


def test_a_pair_of_1000_one_entry_chains_at_chain_borders(ctx):
    rng = np.random.default_rng(7)
    n = 1000
    codes = np.array([EQ, X, EQ, D, EQ, I, I, EQ, D], dtype=np.int64)[np.arange(n) % 9]
    codes[0] = codes[-1] = EQ
    lens = rng.integers(1, 4, n)
    pair = [([int(lens[i]) << 4 | int(codes[i])], int(rng.integers(0, 3)) + (5 if i == 0 else 0), int(rng.integers(0, 3)) + (5 if i == 0 else 0)) for i in range(n)]
    w = world([[("3=", 1, 1)], pair, [("2=1X", 0, 0)]], shuffle=8)
    walker = w[4][1]
    quads = []
    for side in (0, 1):
        s0 = [s[2] if side else s[0] for s in walker.spans]
        s1 = [s[3] if side else s[1] for s in walker.spans]
        for i in range(n):
            for span in (0, 1, 2, 500):
                j = min(i + span, n - 1)
                quads += [(1, side, lo, hi) for lo in (s0[i] - 1, s0[i], s0[i] + 1) for hi in (s1[j] - 1, s1[j], s1[j] + 1) if 0 <= lo < hi]
    quads = quads[::3]                                        # (every third: enough borders, a few seconds of brute force)
    want = [walker.stats(side, lo, hi) for _, side, lo, hi in quads]
    assert len(quads) > 10_000 and max(x[14] for x in want) > 500 and any(x[14] == 0 for x in want) and max(x[10] for x in want) > 50
    check(ctx, w, quads, want, "1 000 one-entry chains")


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_workgroup_seams(ctx, n):
    w = world(SMALL_PAIRS)
    every, stats = every_range(w[4], margin=1)
    pick = [(7 * q) % len(every) for q in range(n)]
    check(ctx, w, [every[p] for p in pick], [stats[p] for p in pick], f"{n} ranges")


def test_257_links(ctx):
    rng = np.random.default_rng(9)
    texts = ("4=2I", "3D2I6=", "2=2D2D1X", "5=1X3I2D4=", "1=")
    pairs, left = [], 257
    while left:
        k = min(int(rng.integers(1, 5)), left)
        pairs.append([(texts[int(rng.integers(0, len(texts)))], int(rng.integers(0, 4)) + (3 if j == 0 else 0), int(rng.integers(0, 4))) for j in range(k)])
        left -= k
    w = world(pairs, shuffle=10)
    assert w[2].size == 257
    quads, want = every_range(w[4], margin=2)
    check(ctx, w, quads[::5], want[::5], "257 links")


def long_entry_case(big):
    "a pair `3=` / `2=<big>=1I2=` (the middle chain, its long entry apart from the `2=` in front of it) / `1D4=`, and the records as formulas"
    pair = [("3=", 2, 2), ([2 << 4 | EQ, big << 4 | EQ, 1 << 4 | I, 2 << 4 | EQ], 1, 3), ("1D4=", 2, 0)]
    a1, b1 = 6, 8                                             # the middle chain: A 6 .. 6 + big + 4, B 8 .. 8 + big + 5
    a2, b2 = a1 + big + 4 + 2, b1 + big + 5                   # the last chain: A a2 .. a2 + 5, B b2 .. b2 + 4
    quads = [(0, 0, 0, a2 + 9), (0, 1, 0, b2 + 9), (0, 0, 4, a2 + 1), (0, 1, 4, b2 + 2), (0, 0, a1 + 1, a2 + 3), (0, 0, a1 + big, a2 - 1)]
    want = [(2, a2 + 5, 2, b2 + 4, big + 11, 0, 1, 1, 3, 3, 1, 1, 0, 2, 3), (2, b2 + 4, 2, a2 + 5, big + 11, 0, 1, 1, 3, 3, 1, 1, 0, 2, 3),
            (4, a2 + 1, 4, b2, big + 5, 0, 1, 1, 3, 3, 1, 1, 0, 2, 3), (4, b2 + 2, 4, a2 + 3, big + 7, 0, 1, 1, 3, 3, 1, 1, 0, 2, 3),
            (a1 + 1, a2 + 3, b1 + 1, b2 + 2, big + 5, 0, 1, 1, 2, 0, 1, 1, 1, 2, 2), (a1 + big, a1 + big + 4, b1 + big, b1 + big + 5, 4, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1)]
    return pair, quads, want


def test_an_entry_longer_than_32_bits_in_a_middle_chain(ctx):
    pair, quads, want = long_entry_case(6)                    # the formulas, against the brute force at a length it can walk
    walker = world([pair])[4][0]
    assert want == [walker.stats(side, lo, hi) for _, side, lo, hi in quads]
    pair, quads, want = long_entry_case(2 ** 32 + 2)
    w = world([pair])
    assert w[4][0] is None
    check(ctx, w, quads, want, "2^32 + 2")


def random_world(seed, n_pairs, n_entries, n_ranges, most=6):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, most + 1, n_pairs)
    chains = random_chains(seed + 1, int(sizes.sum()), n_entries)
    pairs, at = [], 0
    for k in sizes.tolist():
        pairs.append([(chains[at + j], int(rng.integers(0, 30)) * int(rng.integers(0, 2)), int(rng.integers(0, 30)) * int(rng.integers(0, 2))) for j in range(k)])
        at += k
    w = world(pairs, shuffle=seed + 2)
    quads = []
    while len(quads) < n_ranges:
        p, side = int(rng.integers(0, n_pairs)), int(rng.integers(0, 2))
        first, last = hull(w[4][p], side)
        lo, hi = sorted(int(v) for v in rng.integers(max(first - 5, 0), last + 6, 2))
        if lo < hi:
            quads.append((p, side, lo, hi if rng.integers(0, 4) else lo + int(rng.integers(1, 8))))
    return w, quads, [w[4][p].stats(side, lo, hi) for p, side, lo, hi in quads]


def test_random_pairs_and_ranges(ctx):
    w, quads, want = random_world(21, 300, 120, 10_000)
    assert {x[14] for x in want} >= {0, 1, 2, 3, 4, 5, 6} and max(x[10] for x in want) > 20 and any(x[8] + x[9] > 30 for x in want)
    check(ctx, w, quads, want, "300 random pairs")


def test_no_range(ctx):
    from ntsynt_amd.device import NtsError
    w = world(SMALL_PAIRS[:3])
    scans, searches = ctx.timing("lift_pairs_scan")[1], ctx.timing("lift_pairs_search")[1]
    got = check(ctx, w, [], [], "no range")
    assert got.size == 0 and ctx.timing("lift_pairs_search")[1] == searches and ctx.timing("lift_pairs_scan")[1] > scans     # (pass 1 ran, no search)
    nothing = (np.zeros(0, dtype=np.uint64), w[1][:0], w[2][:0], np.zeros(1, dtype=np.uint64))
    check(ctx, nothing, [], [], "nothing at all")
    bad = w[2].copy()
    bad["chain"][1] = 99
    with pytest.raises(NtsError, match="link 1 is no placement"):                           # (the links are still checked)
        ctx.cigar_lift_pairs(w[0], w[1], bad, w[3], ranges_of([]))


def test_small_large_small_in_one_context():
    "docs/design/04_24_call_order.md: a pointer from ws_get is dead after a later request of its name -- L regrows every buffer S made"
    from ntsynt_amd.device import Context
    cases = {"S": random_world(31, 8, 20, 60, most=3), "L": random_world(32, 40, 80, 240, most=5)}
    for f in (0, 1, 2):
        assert cases["L"][0][f].size >= 4 * cases["S"][0][f].size
    ctx = Context(0)
    try:
        for step, size in enumerate(("S", "L", "S", "L", "S")):
            check(ctx, *cases[size], f"step {step}, {size}")
    finally:
        ctx.close()


def refused(ctx, w, quads, code, *words, counts=None, null=False):
    "the call through the library itself: the return code, the message, `stats` untouched.  counts: (n_cigar, n_chains, n_links, n_pairs, n_ranges) other than the arrays'"
    from ntsynt_amd.device import PAIR_STATS_DTYPE
    cigar, recs, links, pair_first = (np.ascontiguousarray(v) for v in w[:4])
    rs = ranges_of(quads)
    stats = np.full(max(rs.size, 1) * PAIR_STATS_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    before = stats.tobytes()
    n = counts or (cigar.size, recs.size, links.size, pair_first.size - 1, rs.size)
    pointers = (None,) * 6 if null else (cigar.ctypes.data, recs.ctypes.data, links.ctypes.data, pair_first.ctypes.data, rs.ctypes.data, stats.ctypes.data)
    rc = ctx.lib.nts_cigar_lift_pairs(ctx.h, pointers[0], int(n[0]), pointers[1], int(n[1]), pointers[2], int(n[2]), pointers[3], int(n[3]), pointers[4], int(n[4]),
                                      pointers[5])
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(x in said for x in words), (rc, said, words)
    assert stats.tobytes() == before
    return said


def test_ranges_of_no_pair_are_refused(ctx):
    w = world(SMALL_PAIRS)
    good = [(0, 0, 3, 9), (1, 1, 0, 8), (3, 1, 12, 13), (6, 0, 0, 1)] * 70                   # (more than one workgroup)
    for bad, at in (((0, 0, 4, 4), 5), ((0, 0, 5, 4), 17), ((7, 0, 0, 1), 256), ((0xFFFFFFFF, 0, 0, 1), 279), ((0, 2, 0, 1), 3), ((0, 0, 0, 2 ** 63), 31),
                    ((0, 0, 2 ** 64 - 1, 0), 2), ((1, 1, 2 ** 63, 2 ** 63 + 1), 0)):
        quads = list(good)
        quads[at] = bad
        quads[-1] = (9, 0, 3, 10)                                                           # (a later offender as well: the smallest one is named)
        refused(ctx, w, quads, -22, f"nts_cigar_lift_pairs: range {at} is no range of a pair")
    check(ctx, w, [(0, 0, 2 ** 63 - 2, 2 ** 63 - 1), (0, 0, 0, 2 ** 63 - 1)], [PB.NONE, w[4][0].stats(0, 0, 100)], "the largest range")


def test_links_that_are_no_placement_are_refused(ctx):
    w = world(SMALL_PAIRS)
    cigar, recs, links, pair_first, _ = w
    some = [(0, 0, 3, 9), (3, 1, 1, 20)]
    assert links.size == 19 and pair_first.tolist() == [0, 1, 3, 7, 10, 13, 16, 19]

    def broken(change):
        bad = links.copy()
        bad["chain"][18] = 99                                 # (a later offender as well: the smallest link is named)
        change(bad)
        return (cigar, recs, bad, pair_first)

    def put(field, at, value):
        def change(bad):
            bad[field][at] = value
        return change

    for change, at in ((put("chain", 5, 19), 5), (put("chain", 4, 0xFFFFFFFF), 4), (put("reserved", 2, 1), 2),
                       (put("chain", 8, 3), 3),                                             # linked twice: the smallest of its links
                       (put("b0", 8, int(links["b0"][8]) - 1), 8),                          # overlap on B with the link in front of it (no open B base)
                       (put("a0", 9, int(links["a0"][9]) - 1), 9),                          # overlap on A (no open A base)
                       (put("a0", 5, 0), 5), (put("b0", 11, 0), 11),                        # disorder
                       (put("a0", 12, 2 ** 63 - 1), 12), (put("b0", 15, 2 ** 63 - 3), 15), (put("a0", 0, 2 ** 64 - 1), 0)):
        refused(ctx, broken(change), some, -22, f"nts_cigar_lift_pairs: link {at} is no placement of its chain")
    first_of_pair = links.copy()                              # the first link of a pair has no link in front of it: pair 1 may start in front of pair 0's end
    first_of_pair["a0"][1] = first_of_pair["b0"][1] = 0
    ctx.cigar_lift_pairs(cigar, recs, first_of_pair, pair_first, ranges_of(some))
    empty = world([[("2=", 1, 1)], [("1X", 0, 0)]])           # a chain without entries may not be linked
    cigar2, recs2, _ = arrays(["2=", [], "1X"])
    links2 = empty[2].copy()
    links2["chain"] = (0, 1)
    refused(ctx, (cigar2, recs2, links2, empty[3]), [(0, 0, 0, 4)], -22, "link 1 is no placement of its chain")
    # entries that are no CIGAR as well: the chain is named first; a range of no pair as well: the link is named first
    off = cigar.copy()
    off[int(recs[2]["first"])] = 3 << 4 | 3
    refused(ctx, (off, recs, broken(put("chain", 5, 19))[2], pair_first), some, -22, "nts_cigar_lift_pairs: the entries of chain 2 are no CIGAR of its lengths")
    refused(ctx, broken(put("chain", 5, 19)), some + [(99, 0, 0, 1)], -22, "link 5 is no placement")


def test_refusals_before_any_launch(ctx):
    w = world(SMALL_PAIRS)
    cigar, recs, links, pair_first, _ = w
    some = [(1, 0, 3, 4)]
    scans = ctx.timing("lift_pairs_scan")[1]
    beyond = recs.copy()
    beyond["n_cig"][18] += 1
    refused(ctx, (cigar, beyond, links, pair_first), some, -22, "nts_cigar_lift_pairs: chain 18", "beyond n_cigar")
    back = recs.copy()
    back["first"][2] = 0
    refused(ctx, (cigar, back, links, pair_first), some, -22, "nts_cigar_lift_pairs: chain 2", "nondecreasing")
    for at, value, named in ((0, 1, 0), (3, 2, 3), (7, 17, 7), (7, 20, 7), (4, 20, 4)):
        bad = pair_first.copy()
        bad[at] = value
        refused(ctx, (cigar, recs, links, bad), some, -22, f"nts_cigar_lift_pairs: pair_first[{named}]", "not nondecreasing from 0 to n_links")
    for counts in ((2 ** 32, 19, 19, 7, 1), (9, 2 ** 32, 19, 7, 1), (9, 19, 2 ** 32, 7, 1), (9, 19, 19, 2 ** 32, 1), (9, 19, 19, 7, 2 ** 32)):
        refused(ctx, w, some, -34, "2^32", counts=counts, null=True)                          # refused before any array is read: null pointers
    huge = recs.copy()
    huge["len_a"][0], huge["len_a"][1] = 2 ** 62, 2 ** 62                                    # together 2^63
    refused(ctx, (cigar, huge, links, pair_first), some, -34, "2^63")
    assert ctx.timing("lift_pairs_scan")[1] == scans

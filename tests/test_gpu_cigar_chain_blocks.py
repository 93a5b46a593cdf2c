"""nts_cigar_chain_blocks (csrc/nts_cigar.inc, Context.cigar_chain_blocks; docs/design/04_28_block_chain.md) against
tests/chain_brute.py in every record, block, text byte and text_first, on CIGARs, chain records and links fabricated in NumPy (no
genome is read): the smallest shapes at which each rule of the definition can break, the worlds of test_gpu_cigar_lift_pairs.py, the
workgroup seams, long entries and 19-digit sizes, every word alignment of the text, text=False, no link, a small, a larger and again
the small case in ONE context, and every refusal with `pairs` untouched.  Every case's expectation is computed on the CPU before the
GPU is called.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import chain_brute as CB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_lift_pairs import SMALL_PAIRS, random_world, world

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
PAIR_FIELDS = ("a0", "a1", "b0", "b1", "eq", "x", "first_block", "n_blocks")
# per pair [(chain, open A bases in front of it, open B bases in front of it)], as test_gpu_cigar_lift_pairs.SMALL_PAIRS
RULES = {
    "one =": [[("1=", 0, 0)]],
    "=X= is one block": [[("2=1X3=", 4, 2)]],
    "leading and trailing I / D are outside the span": [[("2I3D4=1X2D1I", 1, 5)]],
    "a pair of gaps only": [[("3=", 1, 1)], [("2I3D", 2, 2), ("1D", 1, 0)], [("1X", 0, 3)]],
    "a closed seam merges two blocks": [[("3=", 2, 2), ("2X1=", 0, 0)]],
    "seams open on one side and on both": [[("3=", 2, 2), ("2=", 3, 0), ("1=", 0, 4), ("5=", 2, 6)]],
    "D, an open seam, I: ONE gap line": [[("3=2D", 0, 0), ("4I2=", 5, 7)]],
    "D, a closed seam, I: ONE gap line": [[("3=2D", 0, 0), ("4I2=", 0, 0)]],
    "a middle chain without a match column": [[("3=", 1, 1), ("2I", 1, 1), ("3=", 2, 0)], [("2=", 0, 0), ("1D", 0, 0), ("2=", 0, 0)]],
    "end chains without a match column": [[("2D", 3, 3), ("4=", 0, 1), ("1D", 1, 0)], [("1I", 0, 0), ("1=", 0, 0)]],
}


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


def check(ctx, w, what, want=None):
    "the call with and without text against the brute force (or `want` = (pairs, blocks) where no brute force can walk the input)"
    from ntsynt_amd.device import CHAIN_BLOCK_DTYPE, CHAIN_PAIR_DTYPE
    cigar, recs, links, pair_first = w[:4]
    pairs_w, blocks_w = want if want is not None else CB.brute_blocks(cigar, recs, links, pair_first)
    assert CB.identities_hold(pairs_w, blocks_w), what
    text_w, first_w = CB.brute_text(pairs_w, blocks_w)
    pairs, blocks, text, text_first = ctx.cigar_chain_blocks(cigar, recs, links, pair_first)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {links.size} links, {pair_first.size - 1} pairs, {blocks.size} blocks, {text.size} bytes")
    assert pairs.dtype == CHAIN_PAIR_DTYPE and blocks.dtype == CHAIN_BLOCK_DTYPE and text.dtype == np.uint8 and text_first.dtype == np.uint64
    have = list(zip(*(pairs[f].tolist() for f in PAIR_FIELDS))) if pairs.size else []
    assert have == list(pairs_w), (what, [(p, h, x) for p, (h, x) in enumerate(zip(have, pairs_w)) if h != x][:3])
    have = list(zip(*(blocks[f].tolist() for f in ("size", "dt", "dq")))) if blocks.size else []
    assert have == list(blocks_w), (what, [(j, h, x) for j, (h, x) in enumerate(zip(have, blocks_w)) if h != x][:3])
    assert text.tobytes() == text_w and text_first.tolist() == first_w, (what, text.tobytes()[:80], text_w[:80])
    assert not pairs["reserved"].any()
    again = ctx.cigar_chain_blocks(cigar, recs, links, pair_first)
    assert all(g.tobytes() == a.tobytes() for g, a in zip((pairs, blocks, text, text_first), again)), what
    bare = ctx.cigar_chain_blocks(cigar, recs, links, pair_first, text=False)
    assert len(bare) == 2 and bare[0].tobytes() == pairs.tobytes() and bare[1].tobytes() == blocks.tobytes(), what
    return pairs, blocks, text, text_first


@pytest.mark.parametrize("rule", list(RULES))
def test_the_rules_of_the_definition_at_their_smallest(ctx, rule):
    w = world(RULES[rule])
    pairs, blocks, text, _ = check(ctx, w, rule)
    by_hand = {"one =": ([(0, 1, 0, 1, 1, 0, 0, 1)], b"1\n"),
               "=X= is one block": ([(4, 10, 2, 8, 5, 1, 0, 1)], b"6\n"),
               "leading and trailing I / D are outside the span": ([(4, 9, 7, 12, 4, 1, 0, 1)], b"5\n"),
               "a pair of gaps only": ([(1, 4, 1, 4, 3, 0, 0, 1), (0,) * 8, (0, 1, 3, 4, 0, 1, 1, 1)], b"3\n1\n"),
               "a closed seam merges two blocks": ([(2, 8, 2, 8, 4, 2, 0, 1)], b"6\n"),
               "seams open on one side and on both": ([(2, 18, 2, 23, 11, 0, 0, 4)], b"3\t3\t0\n2\t0\t4\n1\t2\t6\n5\n"),
               "D, an open seam, I: ONE gap line": ([(0, 12, 0, 16, 5, 0, 0, 2)], b"3\t7\t11\n2\n"),
               "D, a closed seam, I: ONE gap line": ([(0, 7, 0, 9, 5, 0, 0, 2)], b"3\t2\t4\n2\n"),
               "a middle chain without a match column": ([(1, 10, 1, 10, 6, 0, 0, 2), (0, 5, 0, 4, 4, 0, 2, 2)], b"3\t3\t3\n3\n2\t1\t0\n2\n"),
               "end chains without a match column": ([(5, 9, 4, 8, 4, 0, 0, 1), (0, 1, 1, 2, 1, 0, 1, 1)], b"4\n1\n")}[rule]
    assert list(zip(*(pairs[f].tolist() for f in PAIR_FIELDS))) == by_hand[0] and text.tobytes() == by_hand[1]


def test_chain_records_shuffled_against_link_order(ctx):
    for seed in (1, 2):
        w = world(SMALL_PAIRS + tuple(p for pairs in RULES.values() for p in pairs), shuffle=seed)
        assert not np.array_equal(w[2]["chain"], np.arange(w[2].size))
        check(ctx, w, f"shuffled records, seed {seed}")
    check(ctx, world(SMALL_PAIRS), "the small pairs of the joined lift")


def test_random_worlds(ctx):
    for seed, n_pairs, entries in ((21, 40, 12), (22, 100, 8)):
        w = random_world(seed, n_pairs, entries, 1)[0]
        assert 200 < w[0].size
        _, blocks, _, _ = check(ctx, w, f"random world {seed}")
        assert blocks.size > 100


def seam_pairs(n_blocks):
    "one pair of n_blocks blocks: `1=` chains one open A base apart, and a pair in front of and behind it"
    return [[("2=1D1=", 1, 1)], [("1=", 1, 0)] * n_blocks, [("1X", 0, 0)]]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_workgroup_seams_of_the_blocks(ctx, n):
    pairs, blocks, _, _ = check(ctx, world(seam_pairs(n - 3), shuffle=n), f"{n} blocks")
    assert blocks.size == n and pairs["n_blocks"].tolist() == [2, n - 3, 1]


def test_257_links(ctx):
    rng = np.random.default_rng(9)
    texts = ("4=2I", "3D2I6=", "2=2D2D1X", "5=1X3I2D4=", "1=", "2I", "1D")
    pairs, left = [], 257
    while left:
        k = min(int(rng.integers(1, 5)), left)
        pairs.append([(texts[int(rng.integers(0, len(texts)))], int(rng.integers(0, 3)), int(rng.integers(0, 3))) for _ in range(k)])
        left -= k
    w = world(pairs, shuffle=10)
    assert w[2].size == 257
    check(ctx, w, "257 links")


def test_a_pair_of_1000_one_entry_chains(ctx):
    rng = np.random.default_rng(7)
    n = 1000
    codes = np.array([EQ, X, EQ, D, EQ, I, I, EQ, D], dtype=np.int64)[np.arange(n) % 9]
    lens = rng.integers(1, 4, n)
    pair = [([int(lens[i]) << 4 | int(codes[i])], int(rng.integers(0, 2)) * int(rng.integers(0, 3)), int(rng.integers(0, 2)) * int(rng.integers(0, 3)))
            for i in range(n)]
    pairs, blocks, _, _ = check(ctx, world([[("3=", 1, 1)], pair, [("2=1X", 0, 0)]], shuffle=8), "1 000 one-entry chains")
    assert pairs["n_blocks"][1] > 200 and blocks["size"].max() > 3      # (closed seams merged match runs)


def test_an_entry_longer_than_32_bits_and_a_19_digit_size(ctx):
    def case(big, huge):
        pair = [("3=", 2, 2), ([2 << 4 | EQ, big << 4 | EQ, 1 << 4 | I, 2 << 4 | EQ], 0, 0), ([huge << 4 | X, 3 << 4 | D, huge << 4 | EQ], 2, big)]
        a0 = b0 = 2
        want = ([(a0, a0 + 5 + big + 2 + 2 + huge + 3 + huge, b0, b0 + 5 + big + 1 + 2 + big + 2 * huge, 7 + big + huge, huge, 0, 4)],
                [(5 + big, 0, 1), (2, 2, big), (huge, 3, 0), (huge, 0, 0)])
        return pair, want
    pair, want = case(6, 9)                                   # the formulas, against the brute force at lengths it can walk
    w = world([pair])
    assert CB.brute_blocks(*w[:4]) == want
    pair, want = case(2 ** 32 + 2, 10 ** 18 + 7)              # (10^18 + 7 < 2^60: the longest entry the encoding holds has 19 digits)
    w = world([pair])
    _, _, text, _ = check(ctx, w, "2^32 + 2 and 10^18 + 7", want=want)
    assert text.tobytes() == f"{2 ** 32 + 7}\t0\t1\n2\t2\t{2 ** 32 + 2}\n{10 ** 18 + 7}\t3\t0\n{10 ** 18 + 7}\n".encode()
    # two 19-digit entries in one block and an open stretch of 2^62: numbers beyond 2^60, where the digits come from both halves
    big = 2 ** 60 - 1
    pair = [([big << 4 | EQ, big << 4 | X], 0, 0), ("1=", 2 ** 62, 5)]
    w = world([pair])
    want = ([(0, 2 * big + 2 ** 62 + 1, 0, 2 * big + 6, big + 1, big, 0, 2)], [(2 * big, 2 ** 62, 5), (1, 0, 0)])
    _, _, text, _ = check(ctx, w, "beyond 2^60", want=want)
    assert text.tobytes() == f"{2 * big}\t{2 ** 62}\t5\n1\n".encode()


def test_every_word_alignment_of_the_text(ctx):
    w = world([[("1=", 1, 0)] * 9 + [("1=", 0, 0)]] * 3)      # lines of 2 ("1\n") and 6 bytes
    check(ctx, w, "short lines")
    for lead in (1, 12, 123, 1234):                           # a first line of 2 .. 5 bytes moves every later line through the alignments 0 .. 3
        pair = [(f"{lead}=", 0, 0)] + [(f"{n}=", 0, n) for n in (7, 11, 1, 222, 3, 45, 6, 7777, 8, 9, 10)]
        _, _, text, first = check(ctx, world([[(f"{lead}=", 0, 0)], pair, pair]), f"a first line of {len(str(lead)) + 1} bytes")
        assert int(first[1]) % 4 == (len(str(lead)) + 1) % 4
    threes = world([[("1=", 1, 0)] * 2] * 40)                 # "1\t1\t0\n1\n" per pair; and lines that are all 3 bytes: "10\n"
    check(ctx, threes, "pairs of two lines")
    _, _, text, first = check(ctx, world([[("10=", 0, 0)]] * 41), "lines of 3 bytes")
    assert text.tobytes() == b"10\n" * 41 and first.tolist() == list(range(0, 124, 3))


def test_no_link(ctx):
    from ntsynt_amd.device import NtsError
    w = world(SMALL_PAIRS[:3])
    emits, texts, scans = (ctx.timing(t)[1] for t in ("chain_blocks_emit", "chain_text", "chain_blocks_scan"))
    none = (w[0], w[1], w[2][:0], np.zeros(4, dtype=np.uint64))
    pairs, blocks, text, first = check(ctx, none, "no link", want=([(0,) * 8] * 3, []))
    assert blocks.size == 0 and text.size == 0 and first.tolist() == [0] * 4 and not pairs.tobytes().strip(b"\0")
    assert ctx.timing("chain_blocks_emit")[1] == emits and ctx.timing("chain_text")[1] == texts and ctx.timing("chain_blocks_scan")[1] > scans
    nothing = (np.zeros(0, dtype=np.uint64), w[1][:0], w[2][:0], np.zeros(1, dtype=np.uint64))
    check(ctx, nothing, "nothing at all", want=([], []))
    off = w[0].copy()
    off[0] = 3 << 4 | 3
    with pytest.raises(NtsError, match="the entries of chain 0 are no CIGAR"):        # (the entries are still checked)
        ctx.cigar_chain_blocks(off, *none[1:])


def test_small_large_small_in_one_context():
    "docs/design/04_24_call_order.md: a pointer from ws_get is dead after a later request of its name -- L regrows every buffer S made"
    from ntsynt_amd.device import Context
    cases = {"S": random_world(31, 8, 20, 1, most=3)[0], "L": random_world(32, 40, 80, 1, most=5)[0]}
    ctx = Context(0)
    try:
        for step, size in enumerate(("S", "L", "S", "L", "S")):
            check(ctx, cases[size], f"step {step}, {size}")
    finally:
        ctx.close()


def refused(ctx, w, code, *words, counts=None, null=False):
    "the call through the library itself: the return code, the message, `pairs` and the four results untouched"
    from ntsynt_amd.device import CHAIN_PAIR_DTYPE
    cigar, recs, links, pair_first = (np.ascontiguousarray(v) for v in w[:4])
    n = counts or (cigar.size, recs.size, links.size, pair_first.size - 1)
    pairs = np.full(max(pair_first.size - 1, 1) * CHAIN_PAIR_DTYPE.itemsize, 0xAB, dtype=np.uint8)
    firsts = np.full(pair_first.size, 0xABABABAB, dtype=np.uint64)
    before = (pairs.tobytes(), firsts.tobytes())
    p_blocks, p_text, n_blocks = ctypes.c_void_p(0x1234), ctypes.c_void_p(0x5678), ctypes.c_uint64(77)
    pointers = (None,) * 4 if null else (cigar.ctypes.data, recs.ctypes.data, links.ctypes.data, pair_first.ctypes.data)
    rc = ctx.lib.nts_cigar_chain_blocks(ctx.h, pointers[0], int(n[0]), pointers[1], int(n[1]), pointers[2], int(n[2]), pointers[3], int(n[3]),
                                        pairs.ctypes.data, ctypes.byref(p_blocks), ctypes.byref(n_blocks), ctypes.byref(p_text), firsts.ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(x in said for x in words), (rc, said, words)
    assert (pairs.tobytes(), firsts.tobytes()) == before and (p_blocks.value, p_text.value, n_blocks.value) == (0x1234, 0x5678, 77)
    return said


def test_links_that_are_no_placement_are_refused(ctx):
    w = world(SMALL_PAIRS)
    cigar, recs, links, pair_first, _ = w
    assert links.size == 19 and pair_first.tolist() == [0, 1, 3, 7, 10, 13, 16, 19]

    def broken(field, at, value):
        bad = links.copy()
        bad["chain"][18] = 99                                 # (a later offender as well: the smallest link is named)
        bad[field][at] = value
        return (cigar, recs, bad, pair_first)

    for (field, at, value), named in ((("chain", 5, 19), 5), (("chain", 4, 0xFFFFFFFF), 4), (("reserved", 2, 1), 2),
                                      (("chain", 8, 3), 3),                                             # linked twice: the smallest of its links
                                      (("b0", 8, int(links["b0"][8]) - 1), 8), (("a0", 9, int(links["a0"][9]) - 1), 9),   # overlap
                                      (("a0", 5, 0), 5), (("b0", 11, 0), 11),                         # disorder
                                      (("a0", 12, 2 ** 63 - 1), 12), (("b0", 15, 2 ** 63 - 3), 15), (("a0", 0, 2 ** 64 - 1), 0)):
        refused(ctx, broken(field, at, value), -22, f"nts_cigar_chain_blocks: link {named} is no placement of its chain")
    cigar2, recs2, _ = arrays(["2=", [], "1X"])               # a chain without entries may not be linked
    links2 = world([[("2=", 1, 1)], [("1X", 0, 0)]])[2].copy()
    links2["chain"] = (0, 1)
    refused(ctx, (cigar2, recs2, links2, np.array([0, 1, 2], dtype=np.uint64)), -22, "link 1 is no placement of its chain")
    off = cigar.copy()                                        # entries that are no CIGAR as well: the chain is named first
    off[int(recs[2]["first"])] = 3 << 4 | 3
    refused(ctx, (off, recs, broken("chain", 5, 19)[2], pair_first), -22, "nts_cigar_chain_blocks: the entries of chain 2 are no CIGAR of its lengths")
    short = recs.copy()
    short["len_a"][4] += 1
    refused(ctx, (cigar, short, links, pair_first), -22, "the entries of chain 4 are no CIGAR of its lengths")
    check(ctx, w, "and the same context still answers")


def test_refusals_before_any_launch(ctx):
    w = world(SMALL_PAIRS)
    cigar, recs, links, pair_first, _ = w
    scans = ctx.timing("chain_blocks_scan")[1]
    beyond = recs.copy()
    beyond["n_cig"][18] += 1
    refused(ctx, (cigar, beyond, links, pair_first), -22, "nts_cigar_chain_blocks: chain 18", "beyond n_cigar")
    back = recs.copy()
    back["first"][2] = 0
    refused(ctx, (cigar, back, links, pair_first), -22, "nts_cigar_chain_blocks: chain 2", "nondecreasing")
    for at, value, named in ((0, 1, 0), (3, 2, 3), (7, 17, 7), (7, 20, 7), (4, 20, 4)):
        bad = pair_first.copy()
        bad[at] = value
        refused(ctx, (cigar, recs, links, bad), -22, f"nts_cigar_chain_blocks: pair_first[{named}]", "not nondecreasing from 0 to n_links")
    for counts in ((2 ** 32, 19, 19, 7), (9, 2 ** 32, 19, 7), (9, 19, 2 ** 32, 7), (9, 19, 19, 2 ** 32)):
        refused(ctx, w, -34, "2^32", counts=counts, null=True)                               # refused before any array is read: null pointers
    huge = recs.copy()
    huge["len_a"][0], huge["len_a"][1] = 2 ** 62, 2 ** 62                                    # together 2^63
    refused(ctx, (cigar, huge, links, pair_first), -34, "2^63")
    assert ctx.timing("chain_blocks_scan")[1] == scans

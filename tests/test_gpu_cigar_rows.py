"""nts_cigar_rows (csrc/nts_cigar.inc, Context.cigar_rows; docs/design/04_29_block_maf.md) against tests/maf_brute.py in every byte of both
rows and every row_first, on CIGARs fabricated in NumPy over the two small uploaded genomes of tests/test_gpu_cigar_text.py: chains of 1
to 9 columns (every residue mod 4, a chain border at every offset of a word), four entries of length 1 in one word in every order of
= X I D, a word whose four columns belong to four chains, empty chains first, in the middle, last and two in a row, a single-entry
chain, one `=` run over a whole 1 Mbp record, entries that start at columns 1 023 and 1 024 of the buffer, D and I of 1, 3, 4, 5 and
1 023 bases, indels as a chain's first and last column, neighbouring entries of one kind, chains at base 0 and at the last base of a
record, the second record, an N inside a deletion, an insertion and a match -- each forwards, backwards and mixed; 2 000 random chains of
mixed strands; every refusal, the caller's arrays untouched; and the same bytes after larger and smaller calls and after cigar_build,
cigar_text and cigar_chain_blocks in one context.  Every case's expectation is computed on the CPU before the GPU is called.  Every
test runs under a time limit of its own."""
import ctypes
import faulthandler
import itertools

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import maf_brute as MB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_text import MBP, World, lengths_of, random_specs

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
EINVAL, ERANGE = -22, -34
LETTER = {"I": I, "D": D, "=": EQ, "X": X}


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


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.free()


def case(world, specs):
    """specs: per chain (entries or CIGAR string, rec_a, pos_a, rec_b, start_b, backwards) -- the query bases are start_b .. start_b + len_b
    - 1 of the record, read backwards and complemented for a backward chain.  Returns (cigar, records, spans, rows A, rows B)"""
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    cigar, recs, lists = arrays([s[0] for s in specs])
    spans = np.zeros(len(specs), dtype=CIG_SPAN_DTYPE)
    rows_a, rows_b = [], []
    for c, (_, ra, pa, rb, sb, back) in enumerate(specs):
        la, lb = lengths_of(lists[c])
        assert (la, lb) == (int(recs[c]["len_a"]), int(recs[c]["len_b"]))
        target, query = world.seqs[0][ra][pa:pa + la], world.seqs[1][rb][sb:sb + lb]
        assert len(target) == la and len(query) == lb, "a test chain outside its record"
        spans[c] = (pa, sb + lb - 1 if back and lb else sb, ra, rb, CIG_B_BACKWARDS if back else 0, 0)
        row_a, row_b = MB.rows_from_cigar(lists[c], target, MB.reverse_complement(query) if back else query)
        rows_a.append(row_a)
        rows_b.append(row_b)
    return cigar, recs, spans, rows_a, rows_b


def firsts_of(rows):
    return np.concatenate(([0], np.cumsum([len(t) for t in rows]))).astype(np.uint64)


def same(got, want, first, what):
    assert got.dtype == np.uint8, what
    have, whole = got.tobytes().decode("latin-1"), "".join(want)
    if have != whole:
        at = next(i for i in range(min(len(have), len(whole)) + 1) if have[i:i + 1] != whole[i:i + 1])
        raise AssertionError((what, "first difference at byte", at, have[max(at - 20, 0):at + 20], whole[max(at - 20, 0):at + 20]))
    assert "?" not in have and "\0" not in have, what


def check(ctx, world, specs, what):
    cigar, recs, spans, rows_a, rows_b = case(world, specs)
    got = ctx.cigar_rows(cigar, recs, spans, *world.genomes)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, 2 x {got[0].size} bytes")
    assert len(got) == 3 and got[2].dtype == np.uint64 and np.array_equal(got[2], firsts_of(rows_a)), (what, got[2][:8], firsts_of(rows_a)[:8])
    same(got[0], rows_a, got[2], what + " (row A)")
    same(got[1], rows_b, got[2], what + " (row B)")
    again = ctx.cigar_rows(cigar, recs, spans, *world.genomes)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), what
    return rows_a, rows_b


def both_strands(ctx, world, specs, what):
    "specs without the strand: each case forwards, backwards, and mixed"
    out = [check(ctx, world, [s + (back,) for s in specs], f"{what}, {'backwards' if back else 'forwards'}") for back in (False, True)]
    check(ctx, world, [s + (bool(c % 2),) for c, s in enumerate(specs)], what + ", mixed")
    return out


# ---- word seams ----

def test_chains_of_1_to_9_columns(ctx, world):
    patterns = {1: ["1=", "1X", "1I", "1D"], 2: ["2=", "1I1D", "1D1="], 3: ["3=", "1=1X1I", "3D"], 4: ["4=", "1D3=", "2I2X"], 5: ["5=", "2=1D2=", "4I1="],
                6: ["6=", "3X3D"], 7: ["7=", "3=1I3="], 8: ["8=", "4D4I"], 9: ["9=", "4=1X4=", "1I7=1D"]}
    specs, at, wanted = [], 0, []
    for n in range(1, 10):                                    # every chain length at every offset of a word: a filler of 1 to 3 columns in front where needed
        for j, p in enumerate(patterns[n] + patterns[n][:1]):
            offset = j % 4
            if at % 4 != offset:
                fill = (offset - at) % 4
                specs.append((f"{fill}=", 1, 2 * len(specs), 1, 3 * len(specs)))
                at += fill
            wanted.append((len(specs), offset, n))
            specs.append((p, 0, 10 * n + j, 0, 11 * n + j))
            at += n
    for n in range(1, 10):                                    # (the patterns are fewer than four for some lengths: the first one at the offsets left)
        for offset in range(4):
            if not any(w[1:] == (offset, n) for w in wanted):
                fill = (offset - at) % 4
                if fill:
                    specs.append((f"{fill}X", 1, 2 * len(specs), 1, 3 * len(specs)))
                    at += fill
                wanted.append((len(specs), offset, n))
                specs.append((patterns[n][0], 0, 10 * n + offset, 0, 11 * n + offset))
                at += n
    (rows_a, _), _ = both_strands(ctx, world, specs, "1 to 9 columns")
    starts = firsts_of(rows_a)[:-1]
    assert all((int(starts[c]) % 4, len(rows_a[c])) == (offset, n) for c, offset, n in wanted)
    assert {w[1:] for w in wanted} == {(o, n) for o in range(4) for n in range(1, 10)}
    for n in range(1, 10):                                    # rows that are n columns in all: a buffer of every length from 1 to 9
        for p in patterns[n][:2]:
            check(ctx, world, [(p, 0, 3, 0, 4, False)], f"rows of {n} columns in all")


def test_four_entries_of_length_1_in_one_word_in_every_order(ctx, world):
    orders = list(itertools.permutations("=XID"))
    assert len(orders) == 24
    specs = [("".join("1" + k for k in order), 0, 20 + c, 0, 30 + c) for c, order in enumerate(orders)]
    (rows_a, rows_b), _ = both_strands(ctx, world, specs, "four kinds in one word")
    assert all(len(r) == 4 and r.count("-") == 1 for r in rows_a + rows_b)
    # the same behind 1, 2 and 3 columns: the four entries astride a word border at every offset
    for lead in (1, 2, 3):
        both_strands(ctx, world, [(f"{lead}=", 0, 5, 0, 5)] + specs, f"four kinds behind {lead}")


def test_a_word_whose_four_columns_belong_to_four_chains(ctx, world):
    specs = [("1=", 0, 10, 0, 10), ("1I", 0, 20, 0, 21), ("1D", 0, 30, 0, 31), ("1X", 0, 40, 0, 41),
             ("1D", 1, 0, 1, 0), ([], 0, 0, 0, 0), ("1I", 1, 1199, 1, 1299), ("1X", 0, 2099, 0, 2299), ("1=", 1, 7, 1, 8)]   # (and an empty chain inside a word)
    (rows_a, rows_b), _ = both_strands(ctx, world, specs, "four chains in one word")
    assert [len(r) for r in rows_a] == [1, 1, 1, 1, 1, 0, 1, 1, 1] and rows_a[1] == "-" and rows_b[2] == "-"


# ---- chains ----

def test_single_entry_and_empty_chains(ctx, world):
    both_strands(ctx, world, [("7=", 0, 3, 0, 4)], "one entry")
    specs = [([], 0, 0, 0, 0), ([], 1, 5, 1, 5), ("4=2I1X", 0, 10, 0, 20), ([], 0, 7, 1, 9), ("3D5=", 1, 0, 1, 0), ([], 0, 0, 0, 0), ([], 0, 1, 0, 1),
             ("2X", 0, 50, 0, 60), ([], 1, 1200, 1, 1300)]   # empty: first, two in a row, in the middle, two in a row, last (at a record's end)
    (rows_a, rows_b), _ = both_strands(ctx, world, specs, "empty chains")
    assert [len(t) for t in rows_a] == [0, 0, 7, 0, 8, 0, 0, 2, 0] and rows_a[2][4:6] == "--" and rows_b[4][:3] == "---"
    cigar, recs, spans, _, _ = case(world, [([], 0, 0, 0, 0, False), ([], 0, 0, 0, 0, True)])
    got = ctx.cigar_rows(cigar, recs, spans, *world.genomes)                                # nothing but empty chains: no entry at all
    assert [g.size for g in got] == [0, 0, 3] and not got[2].any()
    got = ctx.cigar_rows(cigar[:0], recs[:0], spans[:0], *world.genomes)                    # and no chain
    assert [g.size for g in got] == [0, 0, 1]


def test_one_run_over_a_whole_record_of_1_mbp(ctx, world):
    (rows_a, rows_b), (_, back_b) = both_strands(ctx, world, [("5=", 0, 0, 0, 0), (f"{MBP}=", 2, 0, 2, 0), ("3I", 1, 4, 1, 4)], "1 Mbp")
    assert rows_a[1] == world.seqs[0][2] and rows_b[1] == world.seqs[1][2] and back_b[1] == MB.reverse_complement(world.seqs[1][2])
    assert rows_a[2] == "---" and len(rows_a[1]) > 900 * 1024                              # (row_first of the last chain: far beyond one workgroup's columns)
    # the same record with a mismatch and an indel at its two ends: base 0 and the last base of a record are read
    both_strands(ctx, world, [(f"1X{MBP - 3}=2D2I", 2, 0, 2, 0), (f"2I2D{MBP - 3}=1X", 2, 0, 2, 0)], "1 Mbp, both ends")


def test_entries_that_start_at_columns_1023_and_1024(ctx, world):
    # across chains: chain 1 is the entry at column 1 023, chain 2 begins at 1 024; inside one chain: 1X at 1 023, 2I at 1 024
    (rows_a, _), _ = both_strands(ctx, world, [("1023=", 0, 30, 0, 40), ("1X", 0, 5, 0, 6), ("5D2=", 1, 3, 1, 4)], "the seam between chains")
    assert firsts_of(rows_a).tolist() == [0, 1023, 1024, 1031]
    (rows_a, _), _ = both_strands(ctx, world, [("1023=1X2I3=1D", 0, 30, 0, 40), ("1000=23D1D5I", 0, 0, 0, 0)], "the seam inside a chain")
    assert rows_a[0][1024:1026] == "--"
    both_strands(ctx, world, [("1020=", 0, 1, 0, 1), ("1=1X1I1D1=1X1I1D", 0, 7, 0, 9)], "four kinds astride the seam")


def test_indels_of_every_size(ctx, world):
    specs = [("3=1X4=5X2=", 0, 100, 0, 200)]
    for n in (1, 3, 4, 5, 1023):
        specs.append((f"2={n}D3={n}I2=", 0, 40, 0, 30))
        specs.append((f"{n}D4={n}I", 0, 7, 0, 9))             # an indel as the first and as the last column
        specs.append((f"{n}I4={n}D", 1, 2, 1, 3))
    (rows_a, rows_b), (_, back_b) = both_strands(ctx, world, specs, "sizes")
    assert rows_b[-3][2:1025] == "-" * 1023 and rows_a[-3][1028:2051] == "-" * 1023 and rows_a[-2].endswith("-" * 1023) and rows_a[-1].startswith("-" * 1023)
    assert rows_b != back_b


def test_neighbouring_entries_of_one_kind(ctx, world):
    (rows_a, rows_b), _ = both_strands(ctx, world, [("3=3=2D2D1X1X2I1I4=", 0, 20, 0, 25), ("1I1I1I", 1, 0, 1, 0), ("1D2D", 1, 9, 1, 9)], "not maximal")
    assert rows_b[0][6:10] == "----" and rows_a[0][12:15] == "---" and rows_a[1] == "---" and rows_b[2] == "---"


def test_record_borders_and_the_second_record(ctx, world):
    la, lb = 1200, 1300                                       # the second records
    specs = [("4=1X2D3=", 0, 0, 0, 0),                        # starts at base 0 of both
             ("3=2I1X", 0, 2100 - 4, 0, 2300 - 6),            # ends at the last base of both
             ("2D5=1X", 1, 0, 1, 0), ("5=1X3D", 1, la - 9, 1, lb - 6),   # the second record, both borders
             (f"{la}D", 1, 0, 1, 17), (f"{lb}I", 1, 5, 1, 0)]  # a whole record deleted, a whole record inserted
    (rows_a, rows_b), (_, back_b) = both_strands(ctx, world, specs, "borders")
    assert rows_a[4] == MB.letters(world.seqs[0][1]) and rows_b[5] == MB.letters(world.seqs[1][1]) and rows_b[4] == "-" * la
    assert back_b[5] == MB.reverse_complement(world.seqs[1][1])


def test_n_inside_a_deletion_an_insertion_and_a_match(ctx, world):
    (rows_a, rows_b), (_, back_b) = both_strands(ctx, world, [("2=5D3=", 0, 596, 0, 10), ("2=5I3=", 0, 10, 0, 596), ("3X", 0, 600, 0, 600),
                                                              ("9=", 0, 597, 0, 597)], "N")
    assert "NNN" in rows_a[0] and "NNN" in rows_b[1] and (rows_a[2], rows_b[2]) == ("NNN", "NNN") and rows_a[3][3:6] == "NNN" == rows_b[3][3:6]
    assert "NNN" in back_b[1] and back_b[2] == "NNN" and back_b[3][3:6] == "NNN"            # (complemented or not, what is no base is N)


def test_random_chains_of_mixed_strands(ctx, world):
    specs = random_specs(77, 2000, 25)
    assert 40_000 < sum(len(s[0]) for s in specs) < 60_000 and any(not s[0] for s in specs)
    rows_a, rows_b = check(ctx, world, specs, "2 000 random chains")
    assert sum(len(t) for t in rows_a) > 300_000


# ---- call order ----

def test_the_same_bytes_after_larger_and_smaller_calls_and_other_entry_points(world):
    "docs/design/04_24_call_order.md: a pointer from ws_get is dead after a later request of its name -- L regrows every buffer S made"
    from ntsynt_amd.device import Context, Genome
    from tests import chain_brute as CB
    from tests.test_gpu_cigar_lift_pairs import random_world
    cases = {size: case(world, random_specs(seed, n, 6)) for size, (seed, n) in (("S", (41, 12)), ("L", (42, 60)))}
    assert cases["L"][0].size >= 4 * cases["S"][0].size
    others = {(name, size): (C.case_of(name, size), C.expected_of(name, size)) for name in ("cigar_build", "cigar_text") for size in C.SIZES}
    blocks_in = {}
    for size, (seed, pairs, entries, ranges, most) in (("S", (51, 8, 20, 60, 3)), ("L", (52, 40, 80, 240, 5))):   # (tests/chain_brute.py is the reference)
        w, _, _ = random_world(seed, pairs, entries, ranges, most=most)
        blocks_in[size] = (w[:4], CB.brute_blocks(*w[:4]))
    ctx = Context(0)
    try:
        genomes = []
        for seqs in world.seqs:                               # (genomes of this context's own)
            sizes = np.array([len(s) for s in seqs], dtype=np.uint64)
            offs = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64)
            genomes.append(Genome(ctx, [f"r{i}" for i in range(len(seqs))], np.frombuffer("".join(seqs).encode(), dtype=np.uint8), offs, sizes))
        first = {}
        for step, size in enumerate(("S", "L", "S", "L", "S")):
            cigar, recs, spans, rows_a, rows_b = cases[size]
            got = ctx.cigar_rows(cigar, recs, spans, *genomes)
            assert np.array_equal(got[2], firsts_of(rows_a)), (step, size)
            same(got[0], rows_a, got[2], f"step {step}, {size} (row A)")
            same(got[1], rows_b, got[2], f"step {step}, {size} (row B)")
            assert first.setdefault(size, [g.tobytes() for g in got]) == [g.tobytes() for g in got], (step, size)
            other = "L" if step % 2 == 0 else "S"
            for name in ("cigar_text", "cigar_build"):        # (sizes that rise and fall between the calls under test)
                assert C.BY_NAME[name].run(ctx, others[(name, other)][0]) == others[(name, other)][1], (step, name, other)
            args, (pairs_w, blocks_w) = blocks_in[other]
            made = ctx.cigar_chain_blocks(*args)
            assert list(zip(*(made[1][f].tolist() for f in ("size", "dt", "dq")))) == blocks_w, (step, "cigar_chain_blocks", other)
            assert list(zip(*(made[0][f].tolist() for f in ("a0", "a1", "b0", "b1", "eq", "x", "first_block", "n_blocks")))) == pairs_w, (step, other)
        for g in genomes:
            g.free()
    finally:
        ctx.close()


# ---- refusals ----

def refused(ctx, world, cigar, recs, spans, code, *words, counts=None, genomes="both"):
    "the call through the library itself: the return code, the message, no buffer returned and the caller's array untouched"
    recs, cigar = np.ascontiguousarray(recs), np.ascontiguousarray(cigar, dtype=np.uint64)
    n = counts or (cigar.size, recs.size)
    first = np.full(max(recs.size, 1) + 1, 0xABABABABABABABAB, dtype=np.uint64)
    before = first.tobytes()
    mark = 0x5A5A5A5A
    p_a, p_b = ctypes.c_void_p(mark), ctypes.c_void_p(mark)
    g_a = world.genomes[0].h if genomes in ("both", "a") else None
    g_b = world.genomes[1].h if genomes in ("both", "b") else None
    rc = ctx.lib.nts_cigar_rows(ctx.h, cigar.ctypes.data, int(n[0]), recs.ctypes.data, int(n[1]), g_a, g_b, spans.ctypes.data if spans is not None else None,
                                ctypes.byref(p_a), ctypes.byref(p_b), first.ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert first.tobytes() == before and p_a.value == mark and p_b.value == mark
    return said


GOOD = [("5=1X3I2D4=", 0, 10, 0, 20, False), ("3D2I6=", 1, 0, 1, 4, True), ([], 0, 0, 0, 0, False), ("4=2I", 0, 2096, 1, 1294, True)]


def test_refusals_before_any_launch(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    scans = ctx.timing("cigar_rows_scan")[1]
    for counts in ((2 ** 32, 4), (10, 2 ** 32), (2 ** 40, 2 ** 40)):                          # before any array is read: 1-element arrays
        refused(ctx, world, cigar[:1].copy(), recs[:1].copy(), spans[:1].copy(), ERANGE, "nts_cigar_rows", "2^32", counts=counts)
    # chains that do not tile the entries: the smallest chain is named
    for field, at, value, chain in (("first", 0, 1, 0), ("first", 1, 4, 1), ("first", 1, 6, 1), ("n_cig", 1, 2, 2), ("n_cig", 3, 1, 3), ("n_cig", 3, 3, 3),
                                    ("first", 2, 2 ** 64 - 1, 2), ("n_cig", 0, 2 ** 64 - 1, 0)):
        bad = recs.copy()
        bad[field][at] = value
        refused(ctx, world, cigar, bad, spans, EINVAL, f"nts_cigar_rows: chain {chain}", "do not tile")
    refused(ctx, world, cigar, recs[:0], spans[:0], EINVAL, "do not tile")                    # entries and no chain
    bad = spans.copy()
    bad["flags"][1], bad["flags"][3] = 3, 2
    refused(ctx, world, cigar, recs, bad, EINVAL, "chain 1 has unknown flag bits")
    for field in ("rec_a", "rec_b"):
        bad = spans.copy()
        bad[field][1], bad[field][3] = 3, 0xFFFFFFFF
        refused(ctx, world, cigar, recs, bad, EINVAL, "chain 1 names a record outside its genome")
    #   pos_a + len_a > rec_len_a; forwards pos_b + len_b > rec_len_b; backwards pos_b >= rec_len_b, len_b > pos_b + 1; len_b = 0: pos_b > rec_len_b
    for chain, field, value in ((0, "pos_a", 2100 - 12 + 1), (0, "pos_a", 2 ** 64 - 1), (0, "pos_b", 2300 - 13 + 1), (0, "pos_b", 2 ** 64 - 5), (1, "pos_b", 1300),
                                (1, "pos_b", 6), (1, "pos_b", 2 ** 64 - 1), (3, "pos_b", 4), (3, "pos_a", 2097), (2, "pos_b", 2301), (2, "pos_a", 2101)):
        bad = spans.copy()
        bad[field][chain] = value
        bad["pos_a"][3] = max(int(bad["pos_a"][3]), 2098)                                   # (a later offender as well)
        refused(ctx, world, cigar, recs, bad, EINVAL, f"nts_cigar_rows: chain {chain}: its span lies outside its record")
    edge = spans.copy()                                                                     # what is still inside
    edge["pos_a"][0], edge["pos_b"][0], edge["pos_b"][1], edge["pos_a"][2], edge["pos_b"][2] = 2100 - 12, 2300 - 13, 7, 2100, 2300
    ctx.cigar_rows(cigar, recs, edge, *world.genomes)
    for which in ("a", "b", "none"):
        refused(ctx, world, cigar, recs, spans, EINVAL, "nts_cigar_rows", "genomes", genomes=which)
    refused(ctx, world, cigar, recs, None, EINVAL, "nts_cigar_rows", "spans")
    huge = recs.copy()
    huge["len_a"][0] = 2 ** 62                                # (in front of chain 0's span check: a length that alone reaches the limit)
    refused(ctx, world, cigar, huge, spans, ERANGE, "2^62")
    huge = recs.copy()
    huge["len_b"][2], huge["len_b"][3] = 2 ** 61, 2 ** 61     # (chain 2 is empty, so its span check passes pos_b <= rec_len_b alone ... and fails: named first)
    refused(ctx, world, cigar, huge, spans, EINVAL, "chain 2: its span lies outside its record")
    assert ctx.timing("cigar_rows_scan")[1] == scans + 1                                   # (the one call that was not refused: `edge`)
    from ntsynt_amd.device import NtsError
    with pytest.raises(ValueError, match="one span per chain"):
        ctx.cigar_rows(cigar, recs, spans[:2], *world.genomes)
    with pytest.raises(NtsError, match="spans and both genomes"):
        ctx.cigar_rows(cigar, recs, spans, world.genomes[0], None)
    with pytest.raises(NtsError, match="do not tile"):
        ctx.cigar_rows(cigar[:-1], recs, spans, *world.genomes)


def test_entries_that_are_no_cigar_are_refused_after_the_scan(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    emits = ctx.timing("cigar_rows_emit")[1]
    assert cigar.size == 10 and [int(r["first"]) for r in recs] == [0, 5, 8, 8]
    for at, value, chain in ((3, 1 << 4 | 3, 0), (7, 2 << 4 | 0, 1), (6, 0 << 4 | I, 1), (0, 0 << 4 | EQ, 0), (9, 7 << 4 | 15, 3), (8, 4 << 4 | 9, 3)):
        bad = cigar.copy()
        bad[9] = 7 << 4 | 15                                 # (a later offender as well: the smallest chain is named)
        bad[at] = value
        refused(ctx, world, bad, recs, spans, EINVAL, f"nts_cigar_rows: the entries of chain {chain} are no CIGAR of its lengths")
    for field in ("len_a", "len_b"):                          # lengths that disagree with the entries
        off = recs.copy()
        off[field][1] = int(off[field][1]) - 1
        off["len_a"][3] -= 1
        refused(ctx, world, cigar, off, spans, EINVAL, "the entries of chain 1 are no CIGAR of its lengths")
    assert ctx.timing("cigar_rows_emit")[1] == emits

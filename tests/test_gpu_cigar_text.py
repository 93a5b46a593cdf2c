"""nts_cigar_text (csrc/nts_cigar.inc, Context.cigar_text; docs/design/04_26_block_paf_cs.md) against tests/cs_brute.py in every byte of
both texts and every first, on CIGARs fabricated in NumPy over small uploaded genomes: numbers of 1 to 19 digits; texts whose lengths
cover every residue mod 4, tokens astride a dword border at every offset, texts of 1 to 7 bytes (2 to 7: a token has two); a
single-entry chain, empty chains first, in the middle, last and two in a row, one `=` run over a whole 1 Mbp record; X runs of 1 and 5,
D and I of 1, 3, 4, 5 and 1 023 bases, indels as a chain's first and last column, neighbouring entries of one kind, chains at base 0 and
at the last base of a record, the second record, an N inside a deletion and an insertion -- each on a forward and on a backward,
complemented query; 2 000 random chains of mixed strands; every refusal, the caller's arrays untouched; and the same bytes after larger
and smaller calls and after cigar_build, cigar_lift and cigar_lift_stats in one context.  Every case's expectation is computed on the CPU
before the GPU is called.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import cs_brute as CS
from tests import lift_stats_brute as SB
from tests.test_gpu_cigar_lift import arrays

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
I, D, EQ, X = 1, 2, 7, 8
EINVAL, ERANGE = -22, -34
MBP = 1_000_000


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


class World:
    "two small genomes on the device and their records as strings: three records each, the third of exactly 1 Mbp, some N in the first two"

    def __init__(self, ctx):
        from ntsynt_amd.device import Genome
        rng = np.random.default_rng(2601)
        self.seqs, self.genomes = [], []
        for lens in ((2100, 1200, MBP), (2300, 1300, MBP)):
            recs = []
            for n in lens:
                s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
                if n < MBP:
                    s[rng.integers(0, n, 12)] = ord("N")
                    s[[0, n - 1]] = ord("A"), ord("G")
                    s[600:603] = ord("N")                     # (a stretch the cases below aim at: bases 600 .. 602)
                recs.append(s.tobytes().decode())
            sizes = np.array(lens, dtype=np.uint64)
            offs = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64)
            self.seqs.append(recs)
            self.genomes.append(Genome(ctx, [f"r{i}" for i in range(len(lens))], np.frombuffer("".join(recs).encode(), dtype=np.uint8), offs, sizes))

    def free(self):
        for g in self.genomes:
            g.free()


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.free()


def lengths_of(entries):
    a = sum(v >> 4 for v in entries if v & 15 in (EQ, X, D))
    b = sum(v >> 4 for v in entries if v & 15 in (EQ, X, I))
    return a, b


def case(world, specs):
    """specs: per chain (entries or CIGAR string, rec_a, pos_a, rec_b, start_b, backwards) -- the query bases are start_b .. start_b + len_b
    - 1 of the record, read backwards and complemented for a backward chain.  Returns (cigar, records, spans, cg texts, cs texts)"""
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    cigar, recs, lists = arrays([s[0] for s in specs])
    spans = np.zeros(len(specs), dtype=CIG_SPAN_DTYPE)
    cg, cs = [], []
    for c, (_, ra, pa, rb, sb, back) in enumerate(specs):
        la, lb = lengths_of(lists[c])
        assert (la, lb) == (int(recs[c]["len_a"]), int(recs[c]["len_b"]))
        target, query = world.seqs[0][ra][pa:pa + la], world.seqs[1][rb][sb:sb + lb]
        assert len(target) == la and len(query) == lb, "a test chain outside its record"
        spans[c] = (pa, sb + lb - 1 if back and lb else sb, ra, rb, CIG_B_BACKWARDS if back else 0, 0)
        cg.append(CS.cg_from_cigar(lists[c]))
        cs.append(CS.cs_from_cigar(lists[c], target, CS.reverse_complement(query) if back else query))
    return cigar, recs, spans, cg, cs


def firsts_of(texts):
    return np.concatenate(([0], np.cumsum([len(t) for t in texts]))).astype(np.uint64)


def same(got_text, got_first, want, what):
    assert got_text.dtype == np.uint8 and got_first.dtype == np.uint64, what
    assert np.array_equal(got_first, firsts_of(want)), (what, got_first[:8], firsts_of(want)[:8])
    have, whole = got_text.tobytes().decode("latin-1"), "".join(want)
    if have != whole:
        at = next(i for i in range(min(len(have), len(whole)) + 1) if have[i:i + 1] != whole[i:i + 1])
        raise AssertionError((what, "first difference at byte", at, have[max(at - 20, 0):at + 20], whole[max(at - 20, 0):at + 20]))


def check(ctx, world, specs, what):
    cigar, recs, spans, cg, cs = case(world, specs)
    got = ctx.cigar_text(cigar, recs, spans, *world.genomes)
    print(f"{what}: {cigar.size} entries, {recs.size} chains, {got[0].size} + {got[2].size} bytes")
    same(got[0], got[1], cg, what + " (cg)")
    same(got[2], got[3], cs, what + " (cs)")
    again = ctx.cigar_text(cigar, recs, spans, *world.genomes)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), what
    alone = ctx.cigar_text(cigar, recs)
    assert len(alone) == 2 and alone[0].tobytes() == got[0].tobytes() and alone[1].tobytes() == got[1].tobytes(), what
    return cg, cs


def both_strands(ctx, world, specs, what):
    "specs without the strand: each case forwards, backwards, and mixed"
    out = [check(ctx, world, [s + (back,) for s in specs], f"{what}, {'backwards' if back else 'forwards'}") for back in (False, True)]
    check(ctx, world, [s + (bool(c % 2),) for c, s in enumerate(specs)], what + ", mixed")
    return out


# ---- cg without spans ----

def test_numbers_of_1_to_19_digits(ctx):
    from ntsynt_amd import assess
    values = sorted({10 ** d - 1 for d in range(1, 19)} | {10 ** d for d in range(0, 19)} | {2 ** 32 + 2, 2 ** 60 - 1, 2 ** 32 - 1, 2 ** 32, 12345678901234567})
    assert {len(str(v)) for v in values} == set(range(1, 20)) and {9, 10, 99, 100} <= set(values)
    codes = (EQ, I, D, X)
    small, big = [v for v in values if v < 10 ** 15], [v for v in values if v >= 10 ** 15]
    chains = [[v << 4 | codes[(i + shift) % 4] for i, v in enumerate(small)] for shift in range(4)]            # every letter behind every number
    chains.append([v << 4 | (D, I)[i % 2] for i, v in enumerate(big)])                      # (the bases of all chains stay below 2^62 a side)
    chains.append([10 ** 18 << 4 | X, (2 ** 60 - 1) << 4 | EQ])
    cigar, recs, lists = arrays(chains)
    assert int(recs["len_a"].sum()) < 2 ** 62 and int(recs["len_b"].sum()) < 2 ** 62
    want = [CS.cg_from_cigar(entries) for entries in lists]
    got = ctx.cigar_text(cigar, recs)
    assert len(got) == 2
    same(got[0], got[1], want, "digits")
    assert want == assess.cigar_texts(cigar, recs["first"], recs["n_cig"])
    assert want[-1] == "1000000000000000000X1152921504606846975=" and "4294967298" in want[0]


# ---- word seams ----

def test_texts_of_every_length_mod_4_and_tokens_astride_every_border(ctx, world):
    # cg tokens of 2, 3, 4 and 5 bytes in every order: every token starts at every offset of a dword and every chain's text ends at one
    tokens = {2: 3 << 4 | EQ, 3: 12 << 4 | X, 4: 345 << 4 | EQ, 5: 1000 << 4 | X}
    chains = []
    for lead in range(0, 8):                                  # `lead` bytes in front, then each token length
        for size in (2, 3, 4, 5):
            head = {0: [], 2: [2], 3: [3], 4: [4], 5: [5], 6: [3, 3], 7: [3, 4], 1: None}[lead]
            if head is not None:
                chains.append([tokens[t] for t in head + [size]])
    cigar, recs, lists = arrays(chains)
    want = [CS.cg_from_cigar(e) for e in lists]
    assert {len(t) % 4 for t in want} == {0, 1, 2, 3} and {sum(len(t) for t in want[:c]) % 4 for c in range(len(want))} == {0, 1, 2, 3}
    got = ctx.cigar_text(cigar, recs)
    same(got[0], got[1], want, "cg seams")
    for n_bytes, chain in ((2, "3="), (3, "12="), (4, "1=1X"), (5, "1=12X"), (6, "12=12X"), (7, "1=1X12=")):   # a whole text of 2 .. 7 bytes
        cigar, recs, lists = arrays([chain])
        got = ctx.cigar_text(cigar, recs)
        assert got[0].size == n_bytes
        same(got[0], got[1], [chain], f"a text of {n_bytes} bytes")
    # cs: a text of 2 .. 7 bytes, and indel tokens of every length from 2 to 9 bytes behind 0 .. 3 bytes
    for n_bytes, chain in ((2, "1="), (3, "1X"), (4, "3D"), (5, "4I"), (6, "2X"), (7, "1X3D")):
        for back in (False, True):
            cg, cs = check(ctx, world, [(chain, 1, 5, 1, 7, back)], f"a cs text of {n_bytes} bytes")
            assert len(cs[0]) == n_bytes
    specs = []
    for lead in ("", "1=", "1X", "2D"):                       # 0, 2, 3, 3 bytes in front; with the chains before them every offset occurs
        for n in range(1, 9):
            specs.append((f"{lead}{n}D{n}I1X", 0, 10 * n, 0, 11 * n))
    out = both_strands(ctx, world, specs, "cs seams")
    assert {sum(len(t) for t in out[0][1][:c]) % 4 for c in range(len(specs))} == {0, 1, 2, 3}


# ---- chains ----

def test_single_entry_and_empty_chains(ctx, world):
    both_strands(ctx, world, [("7=", 0, 3, 0, 4)], "one entry")
    specs = [([], 0, 0, 0, 0), ([], 1, 5, 1, 5), ("4=2I1X", 0, 10, 0, 20), ([], 0, 7, 1, 9), ("3D5=", 1, 0, 1, 0), ([], 0, 0, 0, 0), ([], 0, 1, 0, 1),
             ("2X", 0, 50, 0, 60), ([], 1, 1200, 1, 1300)]   # empty: first, two in a row, in the middle, two in a row, last (at a record's end)
    (cg, cs), _ = both_strands(ctx, world, specs, "empty chains")
    assert [len(t) for t in cs] == [0, 0, 8, 0, 6, 0, 0, 6, 0] and cg[2] == "4=2I1X"
    cigar, recs, spans, _, _ = case(world, [([], 0, 0, 0, 0, False), ([], 0, 0, 0, 0, True)])
    got = ctx.cigar_text(cigar, recs, spans, *world.genomes)                                # nothing but empty chains: no entry at all
    assert [g.size for g in got] == [0, 3, 0, 3] and not got[1].any() and not got[3].any()
    got = ctx.cigar_text(cigar[:0], recs[:0], spans[:0], *world.genomes)                    # and no chain
    assert [g.size for g in got] == [0, 1, 0, 1]


def test_one_run_over_a_whole_record_of_1_mbp(ctx, world):
    (cg, cs), _ = both_strands(ctx, world, [("5=", 0, 0, 0, 0), (f"{MBP}=", 2, 0, 2, 0), ("3I", 1, 4, 1, 4)], "1 Mbp")
    assert cs[1] == ":1000000" and cg[1] == "1000000="
    # the same record with a mismatch and an indel at its two ends: base 0 and the last base of a record are read
    both_strands(ctx, world, [(f"1X{MBP - 3}=2D2I", 2, 0, 2, 0), (f"2I2D{MBP - 3}=1X", 2, 0, 2, 0)], "1 Mbp, both ends")


# ---- cs ----

def test_mismatches_and_indels_of_every_size(ctx, world):
    specs = [("3=1X4=5X2=", 0, 100, 0, 200)]
    for n in (1, 3, 4, 5, 1023):
        specs.append((f"2={n}D3={n}I2=", 0, 40, 0, 30))
        specs.append((f"{n}D4={n}I", 0, 7, 0, 9))             # an indel as the first and as the last column
        specs.append((f"{n}I4={n}D", 1, 2, 1, 3))
    (cg, cs), (_, cs_back) = both_strands(ctx, world, specs, "sizes")
    assert cs[0].count("*") == 6 and cs[1].startswith(":2-") and len(cs[-3]) == 2 + 1 + 1023 + 2 + 1 + 1023 + 2
    assert cs != cs_back


def test_neighbouring_entries_of_one_kind(ctx, world):
    (cg, cs), _ = both_strands(ctx, world, [("3=3=2D2D1X1X2I1I4=", 0, 20, 0, 25), ("1I1I1I", 1, 0, 1, 0), ("1D2D", 1, 9, 1, 9)], "not maximal")
    assert cg[0] == "3=3=2D2D1X1X2I1I4=" and cs[0].startswith(":3:3-") and cs[0].count("-") == 2 and cs[0].count("+") == 2
    assert CS.cigar_of_cs(cs[0]) == "6=4D2X3I4="


def test_record_borders_and_the_second_record(ctx, world):
    la, lb = 1200, 1300                                       # the second records
    specs = [("4=1X2D3=", 0, 0, 0, 0),                        # starts at base 0 of both
             ("3=2I1X", 0, 2100 - 4, 0, 2300 - 6),            # ends at the last base of both
             ("2D5=1X", 1, 0, 1, 0), ("5=1X3D", 1, la - 9, 1, lb - 6),   # the second record, both borders
             (f"{la}D", 1, 0, 1, 17), (f"{lb}I", 1, 5, 1, 0)]  # a whole record deleted, a whole record inserted
    (cg, cs), (_, cs_back) = both_strands(ctx, world, specs, "borders")
    assert cs[4] == "-" + CS.letters(world.seqs[0][1]) and cs[5] == "+" + CS.letters(world.seqs[1][1])
    assert cs_back[5] == "+" + CS.reverse_complement(world.seqs[1][1])


def test_n_inside_a_deletion_and_an_insertion(ctx, world):
    (cg, cs), (_, cs_back) = both_strands(ctx, world, [("2=5D3=", 0, 596, 0, 10), ("2=5I3=", 0, 10, 0, 596), ("3X", 0, 600, 0, 600)], "N")
    assert "nnn" in cs[0] and "nnn" in cs[1] and cs[2] == "*nn*nn*nn"
    assert "nnn" in cs_back[1] and cs_back[2] == "*nn*nn*nn"                                # (complemented or not, what is no base is n)


def random_specs(seed, n_chains, mean_entries):
    rng = np.random.default_rng(seed)
    specs = []
    for _ in range(n_chains):
        entries, last = [], 0
        for _ in range(int(rng.integers(0, 2 * mean_entries + 1))):
            code = int(rng.choice([EQ, EQ, EQ, X, I, D]))
            n = int(rng.integers(1, 40)) if code == EQ else int(rng.integers(1, 4)) if code == X else int(rng.integers(1, 12))
            entries.append(n << 4 | code)
            last = code
        la, lb = lengths_of(entries)
        ra, rb = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        size_a, size_b = (2100, 1200, MBP)[ra], (2300, 1300, MBP)[rb]
        assert la <= size_a and lb <= size_b, last
        specs.append((entries, ra, int(rng.integers(0, size_a - la + 1)), rb, int(rng.integers(0, size_b - lb + 1)), bool(rng.integers(0, 2))))
    return specs


def test_random_chains_of_mixed_strands(ctx, world):
    specs = random_specs(77, 2000, 25)
    assert 40_000 < sum(len(s[0]) for s in specs) < 60_000 and any(not s[0] for s in specs)
    cg, cs = check(ctx, world, specs, "2 000 random chains")
    assert sum(len(t) for t in cs) > 100_000


# ---- call order ----

def test_the_same_bytes_after_larger_and_smaller_calls_and_other_entry_points(world):
    "docs/design/04_24_call_order.md: a pointer from ws_get is dead after a later request of its name -- L regrows every buffer S made"
    from ntsynt_amd.device import LIFT_RANGE_DTYPE, Context, Genome
    cases = {size: case(world, random_specs(seed, n, 6)) for size, (seed, n) in (("S", (41, 12)), ("L", (42, 60)))}
    assert cases["L"][0].size >= 4 * cases["S"][0].size
    others = {(name, size): (C.case_of(name, size), C.expected_of(name, size)) for name in ("cigar_build", "cigar_lift") for size in C.SIZES}
    stats_in = {}
    for size in C.SIZES:
        cigar, recs, lists = arrays(["5=1X3I2D4=", "3D2I6="] * (1 if size == "S" else 8))
        quads = [(c, 0, 1, int(recs[c]["len_a"])) for c in range(recs.size)]
        stats_in[size] = (cigar, recs, np.array(quads, dtype=LIFT_RANGE_DTYPE), [SB.range_stats(lists[c], s, lo, hi) for c, s, lo, hi in quads])
    ctx = Context(0)
    try:
        genomes = []
        for seqs in world.seqs:                               # (genomes of this context's own)
            sizes = np.array([len(s) for s in seqs], dtype=np.uint64)
            offs = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64)
            genomes.append(Genome(ctx, [f"r{i}" for i in range(len(seqs))], np.frombuffer("".join(seqs).encode(), dtype=np.uint8), offs, sizes))
        first = {}
        for step, size in enumerate(("S", "L", "S", "L", "S")):
            cigar, recs, spans, cg, cs = cases[size]
            got = ctx.cigar_text(cigar, recs, spans, *genomes)
            same(got[0], got[1], cg, f"step {step}, {size} (cg)")
            same(got[2], got[3], cs, f"step {step}, {size} (cs)")
            assert first.setdefault(size, [g.tobytes() for g in got]) == [g.tobytes() for g in got], (step, size)
            other = "L" if step % 2 == 0 else "S"
            for name in ("cigar_lift", "cigar_build"):        # (sizes that rise and fall between the calls under test)
                assert C.BY_NAME[name].run(ctx, others[(name, other)][0]) == others[(name, other)][1], (step, name, other)
            s_cigar, s_recs, s_ranges, s_want = stats_in[other]
            stats = ctx.cigar_lift_stats(s_cigar, s_recs, s_ranges)
            assert list(zip(*(stats[f].tolist() for f in SB.FIELDS))) == s_want, (step, "cigar_lift_stats", other)
        for g in genomes:
            g.free()
    finally:
        ctx.close()


# ---- refusals ----

def refused(ctx, world, cigar, recs, spans, code, *words, counts=None, genomes="both"):
    "the call through the library itself: the return code, the message, no buffer returned and the caller's arrays untouched"
    recs, cigar = np.ascontiguousarray(recs), np.ascontiguousarray(cigar, dtype=np.uint64)
    n = counts or (cigar.size, recs.size)
    firsts = np.full((2, max(recs.size, 1) + 1), 0xABABABABABABABAB, dtype=np.uint64)
    before = firsts.tobytes()
    mark = 0x5A5A5A5A
    p_cg, p_cs = ctypes.c_void_p(mark), ctypes.c_void_p(mark)
    g_a = world.genomes[0].h if spans is not None and genomes in ("both", "a") else None
    g_b = world.genomes[1].h if spans is not None and genomes in ("both", "b") else None
    if spans is None and genomes == "unasked":
        g_a, g_b = world.genomes[0].h, world.genomes[1].h
    rc = ctx.lib.nts_cigar_text(ctx.h, cigar.ctypes.data, int(n[0]), recs.ctypes.data, int(n[1]), g_a, g_b, spans.ctypes.data if spans is not None else None,
                                ctypes.byref(p_cg), firsts[0].ctypes.data, ctypes.byref(p_cs), firsts[1].ctypes.data)
    said = ctx.lib.nts_last_error(ctx.h).decode()
    print(rc, said)
    assert rc == code and all(w in said for w in words), (rc, said, words)
    assert firsts.tobytes() == before and p_cg.value == mark and p_cs.value == mark
    return said


GOOD = [("5=1X3I2D4=", 0, 10, 0, 20, False), ("3D2I6=", 1, 0, 1, 4, True), ([], 0, 0, 0, 0, False), ("4=2I", 0, 2096, 1, 1294, True)]


def test_refusals_before_any_launch(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    scans = ctx.timing("cigar_text_scan")[1]
    for counts in ((2 ** 32, 4), (10, 2 ** 32), (2 ** 40, 2 ** 40)):                          # before any array is read: 1-element arrays
        refused(ctx, world, cigar[:1].copy(), recs[:1].copy(), spans[:1].copy(), ERANGE, "nts_cigar_text", "2^32", counts=counts)
        refused(ctx, world, cigar[:1].copy(), recs[:1].copy(), None, ERANGE, "2^32", counts=counts)
    # chains that do not tile the entries: the smallest chain is named, with spans and without
    for field, at, value, chain in (("first", 0, 1, 0), ("first", 1, 4, 1), ("first", 1, 6, 1), ("n_cig", 1, 2, 2), ("n_cig", 3, 1, 3), ("n_cig", 3, 3, 3),
                                    ("first", 2, 2 ** 64 - 1, 2), ("n_cig", 0, 2 ** 64 - 1, 0)):
        bad = recs.copy()
        bad[field][at] = value
        for sp in (spans, None):
            refused(ctx, world, cigar, bad, sp, EINVAL, f"nts_cigar_text: chain {chain}", "do not tile")
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
        refused(ctx, world, cigar, recs, bad, EINVAL, f"nts_cigar_text: chain {chain}: its span lies outside its record")
    edge = spans.copy()                                                                     # what is still inside
    edge["pos_a"][0], edge["pos_b"][0], edge["pos_b"][1], edge["pos_a"][2], edge["pos_b"][2] = 2100 - 12, 2300 - 13, 7, 2100, 2300
    ctx.cigar_text(cigar, recs, edge, *world.genomes)
    for which in ("a", "b", "none"):
        refused(ctx, world, cigar, recs, spans, EINVAL, "nts_cigar_text", "genomes", genomes=which)
    refused(ctx, world, cigar, recs, None, EINVAL, "genomes", genomes="unasked")
    huge = recs.copy()
    huge["len_a"][0], huge["len_a"][1] = 2 ** 61, 2 ** 61
    refused(ctx, world, cigar, huge, None, ERANGE, "2^62")
    assert ctx.timing("cigar_text_scan")[1] == scans + 1                                   # (the one call that was not refused: `edge`)
    from ntsynt_amd.device import NtsError
    with pytest.raises(ValueError, match="one span per chain"):
        ctx.cigar_text(cigar, recs, spans[:2], *world.genomes)
    with pytest.raises(ValueError, match="both genomes"):
        ctx.cigar_text(cigar, recs, spans, world.genomes[0])
    with pytest.raises(NtsError, match="do not tile"):
        ctx.cigar_text(cigar[:-1], recs)


def test_entries_that_are_no_cigar_are_refused_after_the_scan(ctx, world):
    cigar, recs, spans, _, _ = case(world, GOOD)
    emits = ctx.timing("cigar_text_emit")[1]
    assert cigar.size == 10 and [int(r["first"]) for r in recs] == [0, 5, 8, 8]
    for at, value, chain in ((3, 1 << 4 | 3, 0), (7, 2 << 4 | 0, 1), (6, 0 << 4 | I, 1), (0, 0 << 4 | EQ, 0), (9, 7 << 4 | 15, 3), (8, 4 << 4 | 9, 3)):
        bad = cigar.copy()
        bad[9] = 7 << 4 | 15                                 # (a later offender as well: the smallest chain is named)
        bad[at] = value
        for sp in (spans, None):
            refused(ctx, world, bad, recs, sp, EINVAL, f"nts_cigar_text: the entries of chain {chain} are no CIGAR of its lengths")
    for field in ("len_a", "len_b"):
        off = recs.copy()
        off[field][1] = int(off[field][1]) - 1
        off["len_a"][3] -= 1
        refused(ctx, world, cigar, off, spans, EINVAL, "the entries of chain 1 are no CIGAR of its lengths")
    assert ctx.timing("cigar_text_emit")[1] == emits


def test_a_text_of_2_to_the_32_bytes_is_refused_after_the_scan(ctx):
    "one X run whose cs text is 3 n >= 2^32 bytes, over a genome made on the device: the scan runs on one entry, nothing is emitted"
    from ntsynt_amd.device import CIG_SPAN_DTYPE, Genome
    n = (2 ** 32 + 2) // 3
    assert 3 * n >= 2 ** 32 > 3 * (n - 1)
    g = Genome.synth(ctx, n + 16, 1, 5, 5, 0.0)
    try:
        class Both:
            genomes = (g, g)
        emits = ctx.timing("cigar_text_emit")[1]
        cigar, recs, _ = arrays([[n << 4 | X]])
        spans = np.zeros(1, dtype=CIG_SPAN_DTYPE)
        refused(ctx, Both, cigar, recs, spans, ERANGE, "nts_cigar_text", "2^32 bytes")
        assert ctx.timing("cigar_text_emit")[1] == emits
        got = ctx.cigar_text(cigar, recs)                     # the cg text alone is 11 bytes
        assert got[0].tobytes().decode() == f"{n}X"
        cigar, recs, _ = arrays([[(n - 1) << 4 | X]])         # (one column fewer is below the limit by construction: 3 (n - 1) < 2^32; not run: 4 GiB of text)
        assert 3 * int(recs[0]["len_a"]) < 2 ** 32
    finally:
        g.free()

"""The pure host functions of the block variant sites (ntsynt_amd/assess.py; docs/design/04_32_block_variant_sites.md) against
tests/variant_sites_brute.py: the host rendering of one group's alleles (alleles_host, the spot check of block_variant_sites) on the
small shapes of tests/test_gpu_cigar_alleles.py and on random groups, the genotypes of a hand-made three-row group -- a row that ends
at pos, a row that begins at an INS slot, a row inside another row's deletion, a missing row --, and the table text.  No GPU."""
import numpy as np
import pytest

from tests import variant_sites_brute as VB
from tests.lift_brute import parse_cigar

I, D, EQ, X = 1, 2, 7, 8
PARAMS = (21, 16, 31, 4096, 1023, (1500, 255, 6))


def as_arrays(chains):
    "chains: (group, t0, entries).  Returns (entries, CHAIN records, {group, t0})"
    from ntsynt_amd.device import CHAIN_DTYPE, CIG_PAD_AT_DTYPE
    recs, at = np.zeros(len(chains), dtype=CHAIN_DTYPE), np.zeros(len(chains), dtype=CIG_PAD_AT_DTYPE)
    n = 0
    for c, (group, t0, entries) in enumerate(chains):
        recs[c]["first"], recs[c]["n_cig"] = n, len(entries)
        recs[c]["len_a"] = sum(v >> 4 for v in entries if v & 15 != I)
        recs[c]["len_b"] = sum(v >> 4 for v in entries if v & 15 != D)
        at[c] = (group, 0, t0)
        n += len(entries)
    return np.array([v for ch in chains for v in ch[2]], dtype=np.uint64), recs, at


def allele_array(found):
    from ntsynt_amd.device import CIG_ALLELE_DTYPE
    out = np.zeros(len(found), dtype=CIG_ALLELE_DTYPE)
    for i, a in enumerate(found):
        out[i] = a + (0,)
    return out


def host_equals_brute(specs, alts):
    "specs: (t0, CIGAR string or entries) of ONE group; alts: per chain its alt bytes"
    from ntsynt_amd.assess import alleles_host
    chains = [(0, t0, parse_cigar(t) if isinstance(t, str) else list(t)) for t0, t in specs]
    want, _, want_carriers = VB.alleles(chains, alts, 1)
    got = alleles_host(*as_arrays(chains), np.frombuffer(b"".join(alts), dtype=np.uint8))
    have = [tuple(int(v) for v in a) for a in zip(got[0], got[2], got[3], got[4], np.cumsum(got[5]) - got[5], [0] * len(got[0]), got[1], got[5])]
    assert have == want, (have[:4], want[:4])
    assert got[6].tolist() == want_carriers
    return want, want_carriers


def test_the_small_shapes():
    assert host_equals_brute([(100, "5=1X2D3=")], [b"G"]) == ([(105, 1, 0, 0, 0, 0, 1, 1), (106, 2, 1, 0, 1, 0, 2, 1)], [0, 0])
    assert host_equals_brute([(10, "4=2I4=")], [b"AC"]) == ([(14, 2, 0, 0, 0, 0, 3, 1)], [0])
    three, _ = host_equals_brute([(0, "3X1=")], [b"ACG"])
    split, _ = host_equals_brute([(0, [1 << 4 | X, 1 << 4 | X, 1 << 4 | X, 1 << 4 | EQ])], [b"ACG"])
    assert three == split and [a[0] for a in three] == [0, 1, 2]
    assert host_equals_brute([(0, "2=1X2="), (0, "2=1X2=")], [b"T", b"T"]) == ([(2, 1, 0, 0, 0, 0, 1, 2)], [0, 1])
    assert host_equals_brute([(0, "2=1X2="), (0, "2=1X2=")], [b"T", b"C"]) == ([(2, 1, 1, 1, 0, 0, 1, 1), (2, 1, 0, 0, 1, 0, 1, 1)], [1, 0])
    kinds, _ = host_equals_brute([(0, "2=1X2="), (0, "2=3D2="), (0, "2=2I3=")], [b"T", b"", b"GG"])
    assert [(a[0], a[6]) for a in kinds] == [(2, 1), (2, 2), (2, 3)]
    dels, _ = host_equals_brute([(0, "2=5D2="), (0, "2=2D5=")], [b"", b""])
    assert [(a[0], a[1], a[6]) for a in dels] == [(2, 2, 2), (2, 5, 2)]
    aba, carriers = host_equals_brute([(0, "2=2I2=")] * 3, [b"AC", b"GT", b"AC"])
    assert [(a[7], carriers[a[4]:a[4] + a[7]]) for a in aba] == [(2, [0, 2]), (1, [1])]
    assert host_equals_brute([(0, ""), (3, "4=")], [b"", b""]) == ([], [])
    assert host_equals_brute([], []) == ([], [])


def test_an_insertion_that_differs_in_its_last_byte_and_stacked_insertions():
    long = bytes(np.random.default_rng(1).choice(list(b"ACGT"), 1000).tolist())
    found, carriers = host_equals_brute([(0, "2=1000I2=")] * 3, [long, long[:-1] + (b"A" if long[-1:] != b"A" else b"C"), long])
    assert [(a[7], carriers[a[4]:a[4] + a[7]]) for a in found] == [(2, [0, 2]), (1, [1])]
    texts = [b"ACGTACGT", b"ACGTACGA", b"TCGTACGT"]
    found, carriers = host_equals_brute([(0, "2=8I2=")] * 600, [texts[c % 3] for c in range(600)])
    assert [a[7] for a in found] == [200, 200, 200] and carriers[:3] == [0, 3, 6]


def random_group(rng, n_chains):
    "(specs, alts) of one group: core chains at random places with random alt bytes from a small alphabet, so that alleles are shared"
    specs, alts = [], []
    for _ in range(n_chains):
        entries = [int(rng.integers(1, 5)) << 4 | EQ]
        for _ in range(int(rng.integers(0, 6))):
            code = int(rng.choice([X, I, D]))
            if entries[-1] & 15 != EQ:
                entries.append(int(rng.integers(1, 4)) << 4 | EQ)
            entries.append(int(rng.integers(1, 4)) << 4 | code)
        if entries[-1] & 15 != EQ:
            entries.append(int(rng.integers(1, 5)) << 4 | EQ)
        specs.append((int(rng.integers(0, 6)), entries))
        alts.append(bytes(rng.choice(list(b"AC"), VB.byte_counts(entries)[1]).tolist()))
    return specs, alts


def test_random_groups():
    rng = np.random.default_rng(23)
    shared = 0
    for _ in range(30):
        found, _ = host_equals_brute(*random_group(rng, int(rng.integers(1, 14))))
        shared += sum(1 for a in found if a[7] > 1)
    assert shared > 20


# ---- the genotypes: one hand-made group of three rows ----
#   row 1: chain 0 covers [0, 10) with an SNV at 4 and an insertion in slot 6, chain 1 covers [10, 20) -- it begins at 10
#   row 2: chain 2 covers [0, 20) with a deletion of [8, 12)
#   row 3: chain 3 covers [12, 20) with the same SNV base at 14 as chain 1 -- row 3 is missing in front of 12
GROUP = [(0, 0, "4=1X1=2I4="), (0, 10, "4=1X5="), (0, 0, "8=4D8="), (0, 12, "2=1X5=")]
GROUP_ROWS = [1, 1, 2, 3]
GROUP_ALTS = [b"TGG", b"C", b"", b"C"]


def test_the_genotypes_of_the_hand_made_group():
    from ntsynt_amd.assess import variant_site_genotypes
    chains = [(g, t0, parse_cigar(t)) for g, t0, t in GROUP]
    found, _, carriers = VB.alleles(chains, GROUP_ALTS, 1)
    assert [(a[0], a[6], a[1], a[7]) for a in found] == [(4, 1, 1, 1), (6, 3, 2, 1), (8, 2, 4, 1), (14, 1, 1, 2)]
    want = VB.genotypes(found, carriers, chains, GROUP_ROWS, [3])
    assert want == ["10.", "10.", "01.", "101"]                # (8: row 1's chain 0 covers it, row 3 begins at 12; 14: chains 1 and 3 carry it)
    _, recs, at = as_arrays(chains)
    t0 = at["t0"].astype(np.int64)
    got = variant_site_genotypes(allele_array(found), np.array(carriers, dtype=np.uint32), GROUP_ROWS, t0, t0 + recs["len_a"].astype(np.int64), [3],
                                 at["group"].astype(np.int64))
    assert got == want


@pytest.mark.parametrize("specs, rows, alts, say", [
    ([(0, 0, "4=1X5="), (0, 0, "10="), (0, 10, "5=")], [1, 2, 2], [b"T", b"", b""], ["10"]),                 # pos 4 inside row 2's first chain
    ([(0, 0, "4=1X5="), (0, 0, "4="), (0, 5, "5=")], [1, 2, 2], [b"T", b"", b""], ["1."]),                   # a row that ends at pos: [0, 4) and [5, 10)
    ([(0, 0, "4=2I6="), (0, 4, "6=")], [1, 2], [b"AA", b""], ["1."]),                                        # a row that begins at the INS slot: t0 = pos
    ([(0, 0, "4=2I6="), (0, 3, "7=")], [1, 2], [b"AA", b""], ["10"]),                                        # ... and one base earlier
    ([(0, 0, "4=1X5="), (0, 0, "2=6D2=")], [1, 2], [b"T", b""], ["01", "10"]),                               # the DEL at 2; the SNV at 4: a row inside another row's deletion is aligned
    ([(0, 0, "4=1X5=")], [2], [b"T"], [".1"]),                                                               # a missing row
])
def test_the_genotypes_at_the_edges(specs, rows, alts, say):
    from ntsynt_amd.assess import variant_site_genotypes
    chains = [(g, t0, parse_cigar(t)) for g, t0, t in specs]
    order = sorted(range(len(chains)), key=lambda c: (chains[c][0], rows[c], chains[c][1]))
    assert order == list(range(len(chains))), "the test's chains ascend by (group, row, t0)"
    found, _, carriers = VB.alleles(chains, alts, 1)
    want = VB.genotypes(found, carriers, chains, rows, [2])
    kinds = sorted(range(len(found)), key=lambda i: found[i][0])
    assert [want[i] for i in kinds] == say
    _, recs, at = as_arrays(chains)
    t0 = at["t0"].astype(np.int64)
    got = variant_site_genotypes(allele_array(found), np.array(carriers, dtype=np.uint32), rows, t0, t0 + recs["len_a"].astype(np.int64), [2],
                                 at["group"].astype(np.int64))
    assert got == want


def test_genotypes_of_two_groups_with_different_rows():
    from ntsynt_amd.assess import variant_site_genotypes
    chains = [(0, 5, parse_cigar("2=1X2=")), (2, 5, parse_cigar("2=1X2=")), (2, 5, parse_cigar("5=")), (2, 0, parse_cigar("2=1D2="))]
    rows, alts = [1, 1, 2, 3], [b"A", b"A", b"", b""]
    found, first, carriers = VB.alleles(chains, alts, 3)
    assert first == [0, 1, 1, 3]
    want = VB.genotypes(found, carriers, chains, rows, [1, 0, 3])
    assert want == ["1", "..1", "10."]
    _, recs, at = as_arrays(chains)
    t0 = at["t0"].astype(np.int64)
    assert variant_site_genotypes(allele_array(found), np.array(carriers, dtype=np.uint32), rows, t0, t0 + recs["len_a"].astype(np.int64), [1, 0, 3],
                                  at["group"].astype(np.int64)) == want
    assert variant_site_genotypes(allele_array([]), np.zeros(0, dtype=np.uint32), [], [], [], [1], []) == []


def test_the_table_text_of_the_hand_made_group():
    from ntsynt_amd.assess import VARIANT_SITES_COLUMNS, variant_sites_table
    chains = [(g, t0, parse_cigar(t)) for g, t0, t in GROUP]
    found, _, carriers = VB.alleles(chains, GROUP_ALTS, 1)
    types = VB.genotypes(found, carriers, chains, GROUP_ROWS, [3])
    ref, alt = b"A" + b"C" + b"ACGT" + b"G", b"".join(GROUP_ALTS)          # (ref bytes in chain order: chain 0's X, chain 1's X, chain 2's D, chain 3's X)
    groups = [("7", "ref.fa", "chr2", 0, 20, 3)]
    want = VB.table_text(groups, found, ref, alt, types, PARAMS)
    got = variant_sites_table(groups, allele_array(found), np.frombuffer(ref, dtype=np.uint8), np.frombuffer(alt, dtype=np.uint8), types, *PARAMS[:5],
                              ends=PARAMS[5])
    assert got == want
    lines = got.splitlines()
    assert lines[0].split("\t") == list(VARIANT_SITES_COLUMNS) and len(lines) == 6
    assert lines[1] == "chr2\t4\t7\tref.fa\tsnv\t1\tA\tT\t3\t2\t1\t10." and lines[2] == "chr2\t6\t7\tref.fa\tins\t2\t-\tGG\t3\t2\t1\t10."
    assert lines[3] == "chr2\t8\t7\tref.fa\tdel\t4\tACGT\t-\t3\t2\t1\t01." and lines[4] == "chr2\t14\t7\tref.fa\tsnv\t1\tC\tC\t3\t3\t2\t101"
    assert lines[5] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500, ends_max_edits 255, ends_penalty 6"
    narrow = PARAMS[:4] + (0, None)
    assert variant_sites_table(groups, allele_array([]), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), [], *narrow[:5]) == \
        VB.table_text(groups, [], b"", b"", [], narrow) == "\t".join(VARIANT_SITES_COLUMNS) + "\n# k 21, rate 16, band 31, max_len 4096, max_edits 0\n"

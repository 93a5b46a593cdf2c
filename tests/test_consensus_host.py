"""The host side of --block-consensus (ntsynt_amd/assess.py; docs/design/04_33_block_consensus.md) without a GPU: profile_host against
tests/profile_brute.py on the device test's small shapes and on random groups; consensus_sequences, consensus_fasta and profile_table
against the brute force's walk and texts on hand-made columns -- a dropped base, an inserted run, a hole --; and a second, independent
check: the columns of a hand-made three-row group counted over the text of its multi-MAF (tests/multi_maf_brute.py) equal the profile's
tallies on every emitted column and are unanimous on every other."""
import numpy as np

from tests import multi_maf_brute as MM
from tests import profile_brute as PB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups

REF = PB.REF

SHAPES = [
    ("5= 1X 2D 3=", [(0, 100, "5=1X2D3=")], [b"ATG"], [b"G"]),
    ("three chains, one alt byte", [(0, 100, "5=1X5=")] * 3, [b"A"] * 3, [b"G"] * 3),
    ("two alt bytes", [(0, 100, "5=1X5=")] * 2, [b"A"] * 2, [b"G", b"C"]),
    ("C C G over A", [(0, 0, "2=1X2=")] * 3, [b"A"] * 3, [b"C", b"C", b"G"]),
    ("G G C C over A", [(0, 0, "2=1X2=")] * 4, [b"A"] * 4, [b"G", b"G", b"C", b"C"]),
    ("I 3 and I 5", [(0, 100, "4=3I4="), (0, 100, "4=5I4="), (0, 100, "8=")], [b""] * 3, [b"ACG", b"ACGTT", b""]),
    ("a fourth holder", [(0, 100, "4=3I4="), (0, 100, "4=5I4="), (0, 100, "8="), (0, 100, "4=3I4=")], [b""] * 4, [b"ACG", b"ATGTT", b"", b"ACG"]),
    ("foreign sites", [(0, 0, "10=2I10=1X9="), (0, 10, "5="), (0, 5, "5="), (0, 20, "3="), (0, 17, "3="), (0, 6, "2=4D2=")],
     [b"T", b"", b"", b"", b"", b"CCCC"], [b"GGA", b"", b"", b"", b"", b""]),
    ("2I 2D", [(0, 50, "3=2I2D3="), (0, 50, "8=")], [b"AC", b""], [b"GG", b""]),
    ("overlap", [(0, 104, "2=1X1D4="), (0, 100, "6=1X3=")], [b"AC", b"A"], [b"G", b"T"]),
    ("a hole", [(0, 0, "2=1X2="), (0, 100, "2=1X2=")], [b"A", b"C"], [b"G", b"T"]),
    ("bytes that are no base", [(0, 0, "2=1X1=1I2=")] * 3, [b"R"] * 3, [b"a*", b"Y-", b"NN"]),
    ("beyond 2^32", [(0, (1 << 33) + 5, "4=1X2="), (0, (1 << 33) + 7, "2=1X1D1I2=")], [b"A", b"AC"], [b"G", b"GT"]),
    ("= alone", [(0, 5, "9="), (0, 6, "120=")], [b"", b""], [b"", b""]),
]


def host_columns(specs, refs, alts, n_groups):
    "profile_host group by group, as Context.cigar_profile's tuples"
    from ntsynt_amd.assess import profile_host
    cigar, recs, lists = arrays([s[2] for s in specs])
    at = at_of(specs)
    ref_first = np.concatenate(([0], np.cumsum([len(r) for r in refs]))).astype(np.int64)
    alt_first = np.concatenate(([0], np.cumsum([len(a) for a in alts]))).astype(np.int64)
    ref, alt = np.frombuffer(b"".join(refs), dtype=np.uint8), np.frombuffer(b"".join(alts), dtype=np.uint8)
    out = []
    for g in range(n_groups):
        mine = np.flatnonzero(at["group"] == g)
        if mine.size == 0:
            continue
        sub = recs[mine].copy()
        sub["first"] -= recs["first"][mine[0]]
        lo, hi = int(recs["first"][mine[0]]), int(recs["first"][mine[-1]] + recs["n_cig"][mine[-1]])
        cols = profile_host(cigar[lo:hi], sub, at[mine], ref[ref_first[mine[0]]:ref_first[mine[-1] + 1]], alt[alt_first[mine[0]]:alt_first[mine[-1] + 1]])
        assert not cols["reserved"].any() and not cols["group"].any()
        cols["group"] = g
        out += PB.as_tuples(cols)
    return out, lists


def test_profile_host_on_the_small_shapes():
    for what, specs, refs, alts in SHAPES:
        have, lists = host_columns(specs, refs, alts, 1)
        want, _ = PB.columns([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], refs, alts, 1)
        assert have == want, (what, have[:4], want[:4])


def test_profile_host_on_random_groups():
    for seed, letters in ((5, b"AC"), (6, b"ACGTN"), (9, b"ACGT")):
        specs = random_groups(seed, 200, 25)
        lists = arrays([s[2] for s in specs])[2]
        rng = np.random.default_rng(seed + 100)
        refs = [bytes(rng.choice(list(letters), PB.byte_counts(e)[0]).tolist()) for e in lists]
        alts = [bytes(rng.choice(list(letters), PB.byte_counts(e)[1]).tolist()) for e in lists]
        have, _ = host_columns(specs, refs, alts, 25)
        want, _ = PB.columns([(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)], refs, alts, 25)
        assert len(want) > 200 and have == want, (seed, len(have), len(want))


def cols_of(tuples):
    from ntsynt_amd.device import CIG_PROFILE_COL_DTYPE
    out = np.zeros(len(tuples), dtype=CIG_PROFILE_COL_DTYPE)
    for i, (pos, group, sub, aligned, match, gap, n, ref, call) in enumerate(tuples):
        out[i] = (pos, group, sub, aligned, match, gap, n, ord(ref), ord(call), (0,) * 6)
    return out


GROUPS = [(7, "ref.fa", "chr1", 0, 40, 2), (8, "ref.fa", "chr1", 50, 60, 2), (9, "ref.fa", "chr2", 5, 30, 3)]
#          pos, group, sub, aligned, match, gap, n, ref, call
HAND = [(12, 0, REF, 2, 0, 0, (0, 0, 0, 2, 0), "A", "T"),              # a replaced base
        (14, 0, REF, 2, 0, 2, (0, 0, 0, 0, 0), "C", "-"),              # a dropped base
        (15, 0, REF, 2, 1, 1, (0, 0, 0, 0, 0), "G", "G"),              # a deletion the majority does not share
        (17, 0, 0, 2, 0, 0, (0, 0, 2, 0, 0), "-", "G"),                # an inserted run of two in front of base 17, ...
        (17, 0, 1, 2, 0, 0, (0, 2, 0, 0, 0), "-", "C"),
        (17, 0, 2, 2, 0, 1, (1, 0, 0, 0, 0), "-", "-"),                # ... whose third column the majority does not hold
        (17, 0, REF, 2, 0, 0, (2, 0, 0, 0, 0), "T", "A"),              # and the base behind the run replaced
        (25, 0, REF, 1, 0, 0, (0, 1, 0, 0, 0), "A", "A"),              # behind a hole: one chain, the reference wins the tie
        (10, 2, 0, 3, 0, 0, (0, 0, 0, 3, 0), "-", "T"),                # a run at the group's first base
        (29, 2, REF, 3, 0, 3, (0, 0, 0, 0, 0), "T", "-")]              # the group's last base dropped
EXTENTS = [(10, 30), None, (10, 30)]
BASES = ["ACACCGGTACGTACGAACGT", None, "GGGGGCCCCCAAAAATTTTT"]


def test_consensus_sequences_and_both_texts_from_hand_made_columns():
    from ntsynt_amd.assess import consensus_fasta, consensus_sequences, profile_table
    cols, col_first = cols_of(HAND), np.array([0, 8, 8, 10], dtype=np.uint64)
    reference = [np.frombuffer(b.encode(), dtype=np.uint8) if b is not None else None for b in BASES]
    got = consensus_sequences(GROUPS, cols, col_first, EXTENTS, reference)
    assert got == ["ACTCGGGCAACGTACGAACGT", None, "TGGGGGCCCCCAAAAATTTT"]
    assert got == [PB.consensus(HAND, g, e, BASES[g]) if e is not None else None for g, e in enumerate(EXTENTS)]
    assert reference[0].tobytes().decode() == BASES[0], "the caller's bytes are not patched"
    text = consensus_fasta(GROUPS, cols, col_first, EXTENTS, reference)
    assert text == PB.fasta_text(GROUPS, HAND, EXTENTS, BASES)
    assert text.splitlines()[0] == ">block_7 ref.fa.chr1:10-30 rows=2 columns=8 changed=5" and text.splitlines()[2] == ">block_9 ref.fa.chr2:10-30 rows=3 columns=2 changed=2"
    for params in ((24, 8, 31, 4000, 0, None), (24, 8, 31, 4000, 1023, (3000, 200, 3))):
        table = profile_table(GROUPS, cols, col_first, *params[:4], max_edits=params[4], ends=params[5])
        assert table == PB.table_text(GROUPS, HAND, params)
    lines = table.splitlines()
    assert lines[1].split("\t") == ["chr1", "12", ".", "7", "ref.fa", "2", "3", "A", "1", "0", "0", "2", "0", "0", "T"]
    assert lines[6].split("\t") == ["chr1", "17", "2", "7", "ref.fa", "2", "3", "-", "1", "0", "0", "0", "0", "2", "-"]
    assert all(sum(map(int, ln.split("\t")[8:14])) == int(ln.split("\t")[6]) for ln in lines[1:-1]) and lines[-1].startswith("# k 24")
    none = consensus_fasta(GROUPS[:1], cols[:0], np.zeros(2, dtype=np.uint64), [None], [None])
    assert none == "" and profile_table(GROUPS[:1], cols[:0], np.zeros(2, dtype=np.uint64), 24, 8, 31, 4000).count("\n") == 2


def test_the_tallies_equal_column_counts_over_the_multi_maf_text():
    rng = np.random.default_rng(11)
    target = "".join(rng.choice(list("ACGT"), 60).tolist())
    # three rows beside the reference; no sub-block in which a row is `-` alone (the multi-MAF leaves such rows out)
    rows = [(1, 5, "6=1X3=2I4=1X3D6=1X4="), (2, 5, "6=1X3=3I2=2X2=2D8=1I3="), (3, 5, "6=1X3=2I5=1D5=1X7=")]
    lists = arrays([r[2] for r in rows])[2]
    sites = MM.widths([(0, t0, e) for (_, t0, _), e in zip(rows, lists)])[0]
    chains, refs, alts, specs = [], [], [], []
    for (row, t0, _), entries in zip(rows, lists):
        t1 = t0 + MM.len_a(entries)
        query, at = [], t0
        for v in entries:                                     # a query that agrees with the CIGAR: = copies, X and I differ from the target
            code, size = v & 15, v >> 4
            for j in range(size):
                if code == PB.EQ:
                    query.append(target[at + j])
                elif code == PB.X:
                    query.append("ACGT"[("ACGT".index(target[at + j]) + 1 + (at + j) % 2) % 4])
                elif code == PB.I:
                    query.append("ACGT"[(row + j) % 3])
            at += size if code != PB.I else 0
        query = "".join(query)
        row_a, row_b = MM.padded_rows(MM.pad_chain(entries, t0, sites), target[t0:t1], query)
        plain_a, plain_b = MM.padded_rows(entries, target[t0:t1], query)
        ref, alt, col = [], [], 0
        for v in entries:
            for _ in range(v >> 4):
                ref += [plain_a[col]] if v & 15 in (PB.X, PB.D) else []
                alt += [plain_b[col]] if v & 15 in (PB.X, PB.I) else []
                col += 1
        refs.append("".join(ref).encode())
        alts.append("".join(alt).encode())
        specs.append((0, t0, entries))
        chains.append(dict(row=row, t0=t0, t1=t1, name=f"q{row}.chr1", src_size=len(query), minus=False, start=0, row_a=row_a, row_b=row_b))
    want, _ = PB.columns(specs, refs, alts, 1)
    emitted = {(c[0], c[2]): c for c in want}
    assert any(c[2] != REF for c in want) and any(c[8] != c[7] for c in want)
    seen, blocks = set(), MM.parse(MM.table([("ref.chr1", len(target), chains, sites)]))
    assert len(blocks) >= 1 and all(len(b) == 4 for b in blocks), "every row takes part in every sub-block"
    for block in blocks:
        pos, sub = block[0][1], 0
        for col in range(len(block[0][5])):
            letters = [r[5][col] for r in block]
            key = (pos, sub) if letters[0] == "-" else (pos, REF)
            counted = [letters.count(s) for s in PB.SYMBOLS]
            if key in emitted:
                assert counted == PB.tallies(emitted[key]), (key, counted, emitted[key])
                seen.add(key)
            else:
                assert len(set(letters)) == 1, (key, letters)
            pos, sub = (pos, sub + 1) if letters[0] == "-" else (pos + 1, 0)
    assert seen == set(emitted)
    have, _ = host_columns([(0, t0, e) for _, t0, e in specs], refs, alts, 1)
    assert have == want

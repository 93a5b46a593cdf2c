"""The pure host functions of the block conservation (ntsynt_amd/assess.py; docs/design/04_31_block_conservation.md) against
tests/conservation_brute.py on hand-made segments and chains: the summary, both texts, the histograms' sums, the host rendering of the
segments (depth_segments_host, the spot check of block_conservation), and the definition itself against column counting over the
multi-MAF text of one three-row group (tests/multi_maf_brute.py).  No GPU."""
import numpy as np
import pytest

from tests import conservation_brute as CB
from tests import multi_maf_brute as MM
from tests.lift_brute import parse_cigar

I, D, EQ, X = 1, 2, 7, 8
PARAMS = (21, 16, 31, 4096, 1023, (1500, 255, 6))
GROUPS = [("3", "ref.fa", "chr1", 100, 200, 2), ("7", "ref.fa", "chr2", 0, 50, 3), ("12", "ref.fa", "chr2", 900, 950, 1)]
#        start, end, group, aligned, match, gap
SEGS = [(100, 130, 0, 2, 2, 0), (130, 131, 0, 2, 1, 0), (131, 140, 0, 2, 1, 1), (140, 150, 0, 1, 1, 0), (160, 200, 0, 2, 0, 0),
        (0, 10, 1, 3, 3, 0), (10, 12, 1, 3, 2, 1), (12, 20, 1, 2, 2, 0), (20, 50, 1, 1, 0, 1)]


def seg_array(segs):
    from ntsynt_amd.device import CIG_DEPTH_SEG_DTYPE
    out = np.zeros(len(segs), dtype=CIG_DEPTH_SEG_DTYPE)
    for i, s in enumerate(segs):
        out[i] = s
    return out


def first_of(segs, n_groups):
    return np.array([sum(1 for s in segs if s[2] < g) for g in range(n_groups + 1)], dtype=np.uint64)


def test_summary_of_hand_made_segments():
    from ntsynt_amd.assess import conservation_summary
    got = conservation_summary(seg_array(SEGS), first_of(SEGS, 3), [2, 3, 1])
    assert got == [{"covered": 90, "core": 80, "conserved": 30, "by_aligned": [10, 80], "by_match": [40, 10, 30]},
                   {"covered": 50, "core": 12, "conserved": 10, "by_aligned": [30, 8, 12], "by_match": [0, 0, 2, 10]},
                   {"covered": 0, "core": 0, "conserved": 0, "by_aligned": [0], "by_match": [0, 0]}]
    assert got == CB.summary(SEGS, 3, [2, 3, 1])
    for s in got:
        assert sum(s["by_aligned"]) == s["covered"] and sum(s["by_match"]) == s["core"] == s["by_aligned"][-1] and s["by_match"][-1] == s["conserved"]
    assert conservation_summary(seg_array([]), first_of([], 2), [2, 0]) == CB.summary([], 2, [2, 0])
    assert conservation_summary(seg_array([]), first_of([], 0), []) == []
    with pytest.raises(ValueError):
        conservation_summary(seg_array(SEGS), first_of(SEGS, 3), [1, 3, 1])     # (aligned 2 in a group of one row)
    with pytest.raises(ValueError):
        conservation_summary(seg_array(SEGS), first_of(SEGS, 3), [2, 3])


def test_both_texts_of_hand_made_segments():
    from ntsynt_amd.assess import CONSERVATION_BED_COLUMNS, conservation_bed, conservation_table
    bed = conservation_bed(GROUPS, seg_array(SEGS), first_of(SEGS, 3), *PARAMS[:5], ends=PARAMS[5])
    assert bed == CB.bed_text(GROUPS, SEGS, PARAMS)
    lines = bed.splitlines()
    assert lines[0] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500, ends_max_edits 255, ends_penalty 6"
    assert lines[3] == "chr1\t131\t140\t3\tref.fa\t2\t2\t1\t0\t1" and lines[-1] == "chr2\t20\t50\t7\tref.fa\t3\t1\t0\t0\t1" and len(lines) == 1 + len(SEGS)
    assert len(CONSERVATION_BED_COLUMNS) == len(lines[1].split("\t")) == 10
    table = conservation_table(GROUPS, seg_array(SEGS), first_of(SEGS, 3), *PARAMS[:5], ends=PARAMS[5])
    assert table == CB.table_text(GROUPS, SEGS, PARAMS)
    lines = table.splitlines()
    assert lines[0] == "block_id\tgenome\tcontig\tstart\tend\trows\tcovered\tcore\tconserved\tby_aligned\tby_match"
    assert lines[1] == "3\tref.fa\tchr1\t100\t200\t2\t90\t80\t30\t10,80\t40,10,30" and lines[3] == "12\tref.fa\tchr2\t900\t950\t1\t0\t0\t0\t0\t0,0"
    assert lines[-1] == bed.splitlines()[0] and len(lines) == 5
    narrow = PARAMS[:4] + (0, None)
    assert conservation_bed(GROUPS, seg_array([]), first_of([], 3), *narrow[:5]) == "# k 21, rate 16, band 31, max_len 4096, max_edits 0\n" == \
        CB.bed_text(GROUPS, [], narrow)
    assert conservation_table(GROUPS, seg_array([]), first_of([], 3), *narrow[:5]) == CB.table_text(GROUPS, [], narrow)


def chains_as_arrays(chains):
    from ntsynt_amd.device import CHAIN_DTYPE, CIG_PAD_AT_DTYPE
    recs, at = np.zeros(len(chains), dtype=CHAIN_DTYPE), np.zeros(len(chains), dtype=CIG_PAD_AT_DTYPE)
    n = 0
    for c, (group, t0, entries) in enumerate(chains):
        recs[c]["first"], recs[c]["n_cig"], recs[c]["len_a"], recs[c]["len_b"] = n, len(entries), MM.len_a(entries), MM.len_b(entries)
        at[c] = (group, 0, t0)
        n += len(entries)
    return np.array([v for ch in chains for v in ch[2]], dtype=np.uint64), recs, at


@pytest.mark.parametrize("texts", [[(100, "5=1X2D3=")], [(10, "4=2I4=")], [(0, "3X2X")], [(5, "2D3=1D")], [(0, "10="), (5, "10X")],
                                   [(0, "5="), (5, "5=")], [(0, "5="), (5, "5X")], [(0, "5="), (8, "5=")], [(3, ""), (4, "2I"), (0, "2=")],
                                   [((1 << 33) + 5, "4=1X"), ((1 << 33) + 7, "4=")], [(7, "")], []])
def test_the_host_rendering_equals_the_brute_force(texts):
    from ntsynt_amd.assess import depth_segments_host
    chains = [(0, t0, parse_cigar(t)) for t0, t in texts]
    want, _ = CB.segments(chains, 1)
    got = depth_segments_host(*chains_as_arrays(chains))
    assert [tuple(int(v) for v in s) for s in zip(got[0], got[1], [0] * len(got[0]), got[2], got[3], got[4])] == want


def test_the_host_rendering_of_random_groups_equals_the_brute_force():
    from ntsynt_amd.assess import depth_segments_host
    rng = np.random.default_rng(17)
    for _ in range(20):
        chains = []
        for _ in range(int(rng.integers(1, 12))):
            entries = [int(rng.integers(1, 9)) << 4 | int(rng.choice([EQ, EQ, X, I, D])) for _ in range(int(rng.integers(0, 10)))]
            chains.append((0, int(rng.integers(0, 40)), entries))
        want, _ = CB.segments(chains, 1)
        got = depth_segments_host(*chains_as_arrays(chains))
        assert [tuple(int(v) for v in s) for s in zip(got[0], got[1], [0] * len(got[0]), got[2], got[3], got[4])] == want


def test_the_triples_equal_column_counting_over_the_multi_maf_text():
    "one three-row group without N: what the definition counts per reference base is what the star alignment's columns show"
    rng = np.random.default_rng(3)
    reference = "".join(rng.choice(list("ACGT"), 80))
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    specs = [(1, 5, "10=2I5=1X3D20=4X6="), (2, 0, "20=3D4=5I10=2X8="), (2, 60, "6=1I2X9="), (3, 12, "8=1X1I1X30=2D7=")]
    chains = []
    for row, t0, text in specs:
        entries, p, query = parse_cigar(text), t0, []
        for v in entries:
            code, size = v & 15, v >> 4
            if code == I:
                query.append("".join(rng.choice(list("ACGT"), size)))
            else:
                query.append("" if code == D else reference[p:p + size] if code == EQ else "".join(other[b] for b in reference[p:p + size]))
                p += size
        chains.append(dict(row=row, t0=t0, t1=p, name=f"q{row}.chr1", src_size=1000, minus=False, start=100 * len(chains), entries=entries,
                           a=reference[t0:p], b="".join(query)))
    sites = MM.widths([(0, c["t0"], c["entries"]) for c in chains])[0]
    for c in chains:
        c["row_a"], c["row_b"] = MM.padded_rows(MM.pad_chain(c["entries"], c["t0"], sites), c["a"], c["b"])
    counted = {}
    for block in MM.parse(MM.MAF_HEADER + MM.group_blocks("ref.chr1", len(reference), chains, sites)):
        p = block[0][1]
        for col, base in enumerate(block[0][5]):
            if base == "-":
                continue
            mine = [r[5][col] for r in block[1:]]
            assert (0, p) not in counted
            counted[(0, p)] = [len(mine), sum(b == base for b in mine), sum(b == "-" for b in mine)]
            p += 1
    want = CB.triples([(0, c["t0"], c["entries"]) for c in chains])
    assert counted == want and len(want) == 77 and {t[0] for t in want.values()} == {1, 2, 3} and any(t[2] for t in want.values())
    from ntsynt_amd.assess import depth_segments_host
    got = depth_segments_host(*chains_as_arrays([(0, c["t0"], c["entries"]) for c in chains]))
    segs, _ = CB.segments([(0, c["t0"], c["entries"]) for c in chains], 1)
    assert [tuple(int(v) for v in s) for s in zip(got[0], got[1], [0] * len(got[0]), got[2], got[3], got[4])] == segs

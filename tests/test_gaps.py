"""The host half of the gap report (ntsynt_amd/gaps.py): cut() on hand-written block tables with the expected rows written out, its
invariants on every block table and .fai under tests/golden/, and the formatting of both files.  No GPU, no library."""
import os

import pytest

from ntsynt_amd import gaps
from ntsynt_amd.assess import BlockRow, read_blocks
from ntsynt_amd.gaps import Gap, Merged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "block_stats")
CELEGANS3 = ["celegans-chrII-III.A.fa.fai", "celegans-chrII-III.B.fa.fai", "celegans-chrII-III.fa.fai"]
CELEGANS2 = ["celegans-chrII-III.A.fa.fai", "celegans-chrII-III.fa.fai"]
TABLES = {
    "celegans-A-B": (GOLDEN, "celegans-A-B-ntSynt.synteny_blocks.tsv", CELEGANS3),
    "celegans-A-B-pre": (GOLDEN, "celegans-A-B-ntSynt.pre-collinear-merge.synteny_blocks.tsv", CELEGANS3),
    "celegans-A": (GOLDEN, "celegans-A-ntSynt.synteny_blocks.tsv", CELEGANS2),
    "celegans-A-pre": (GOLDEN, "celegans-A-ntSynt.pre-collinear-merge.synteny_blocks.tsv", CELEGANS2),
    "celegans-A-with-absent-B": (GOLDEN, "celegans-A-ntSynt.synteny_blocks.tsv", CELEGANS3),
    "three_missing": (CASES, "three_missing.synteny_blocks.tsv", ["three_a.fa.fai", "three_b.fa.fai", "three_c.fa.fai"]),
    "unequal": (CASES, "unequal.synteny_blocks.tsv", ["unequal_big.fa.fai", "unequal_small.fa.fai"]),
    "single": (CASES, "single.synteny_blocks.tsv", ["single_x.fa.fai", "single_y.fa.fai"]),
}


def _b(bid, genome, contig, start, end):
    return BlockRow(str(bid), genome, contig, start, end, "+", "10", "None")


def test_overlapping_and_touching_blocks_a_clipped_block_and_a_record_without_one():
    records = {"g": [("c1", 1000), ("c2", 500), ("c3", 0), ("c4", 300)]}
    blocks = [_b(7, "g", "c1", 600, 700),        # file order is not position order
              _b(1, "g", "c1", 100, 200),
              _b(2, "g", "c1", 150, 300),        # overlaps block 1 and ends the run
              _b(3, "g", "c1", 300, 400),        # touches block 2: one run 100..400
              _b(4, "g", "c1", 320, 400),        # ends where block 3 ends: block 3 is first in the file
              _b(5, "g", "c1", 600, 650),        # starts where block 7 starts: block 7 is first in the file
              _b(6, "g", "c1", 900, 1200),       # clipped at the record's end: no trailing gap
              _b(8, "g", "c4", 0, 100),          # starts at 0: no leading gap
              _b(9, "g", "c4", 100, 100)]        # empty: no block at all
    got_gaps, got_merged = gaps.cut(blocks, records)
    assert got_gaps == [Gap("g", "c1", 0, 100, "leading", ".", "1"),
                        Gap("g", "c1", 400, 600, "between", "3", "7"),
                        Gap("g", "c1", 700, 900, "between", "7", "6"),
                        Gap("g", "c2", 0, 500, "unplaced", ".", "."),
                        Gap("g", "c4", 100, 300, "trailing", "8", ".")]          # (c3 has no base: a gap of length zero is dropped)
    assert got_merged == [Merged("g", "c1", 100, 400), Merged("g", "c1", 600, 700), Merged("g", "c1", 900, 1000), Merged("g", "c4", 0, 100)]


def test_a_genome_absent_from_the_table_non_numeric_ids_and_the_order_of_genomes():
    records = {"zeta": [("s", 50)], "alpha": [("x", 100), ("y", 40)], "mid": [("only", 10)]}
    blocks = [_b("blk-b", "zeta", "s", 10, 20), _b("blk-a", "zeta", "s", 30, 50), _b("blk-a", "alpha", "y", 0, 40), _b("7x", "alpha", "x", 20, 30)]
    got_gaps, got_merged = gaps.cut(blocks, records)
    assert got_gaps == [Gap("alpha", "x", 0, 20, "leading", ".", "7x"), Gap("alpha", "x", 30, 100, "trailing", "7x", "."),
                        Gap("mid", "only", 0, 10, "unplaced", ".", "."),
                        Gap("zeta", "s", 0, 10, "leading", ".", "blk-b"), Gap("zeta", "s", 20, 30, "between", "blk-b", "blk-a")]
    assert got_merged == [Merged("alpha", "x", 20, 30), Merged("alpha", "y", 0, 40), Merged("zeta", "s", 10, 20), Merged("zeta", "s", 30, 50)]
    with pytest.raises(ValueError, match="names genome other"):
        gaps.cut([_b(1, "other", "s", 0, 5)], records)
    with pytest.raises(ValueError, match="names record nope"):
        gaps.cut([_b(1, "mid", "nope", 0, 5)], records)


@pytest.mark.parametrize("case", sorted(TABLES))
def test_gaps_and_blocks_tile_every_record_of_the_golden_tables(case):
    d, tsv, fais = TABLES[case]
    blocks = read_blocks(os.path.join(d, tsv))
    records = {f[:-len(".fai")]: gaps.read_fai(os.path.join(d, f)) for f in fais}
    assert blocks and all(records.values())
    got_gaps, got_merged = gaps.cut(blocks, records)
    covered = {}
    for r in got_gaps + got_merged:
        assert r.end > r.start >= 0
        covered.setdefault((r.genome, r.contig), []).append((r.start, r.end, isinstance(r, Gap)))
    for genome, recs in records.items():
        for contig, length in recs:
            rows = sorted(covered.get((genome, contig), []))
            assert sum(e - s for s, e, _ in rows) == length, (genome, contig)
            at = 0
            for (s, e, is_gap), nxt in zip(rows, rows[1:] + [None]):
                assert s == at, (genome, contig, s, at)                                   # no overlap, no hole
                assert nxt is None or not (is_gap and nxt[2]), (genome, contig, s)       # two gaps never touch
                at = e
            assert at == length
    # every block lies inside the merged intervals of its record, none of it inside a gap
    for b in blocks:
        length = dict(records[b.genome])[b.contig]
        s, e = max(b.start, 0), min(b.end, length)
        assert any(m.genome == b.genome and m.contig == b.contig and m.start <= s and e <= m.end for m in got_merged), b
        assert not any(g.genome == b.genome and g.contig == b.contig and g.start < e and s < g.end for g in got_gaps), b
    # stated order: genomes ascending, records in file order, gaps by start
    order = {(g, c): (gi, ci) for gi, g in enumerate(sorted(records)) for ci, (c, _) in enumerate(records[g])}
    keys = [order[(g.genome, g.contig)] + (g.start,) for g in got_gaps]
    assert keys == sorted(keys)
    ids = {b.block_id for b in blocks}
    for g in got_gaps:
        assert (g.kind == "unplaced") == (g.left_block == "." and g.right_block == "." and g.start == 0)
        assert g.left_block in ids | {"."} and g.right_block in ids | {"."}
        assert (g.kind == "leading") == (g.left_block == "." and g.right_block != ".")
        assert (g.kind == "trailing") == (g.left_block != "." and g.right_block == ".")
        if g.left_block != ".":
            assert any(b.block_id == g.left_block and b.genome == g.genome and b.contig == g.contig and b.end == g.start for b in blocks)
        if g.right_block != ".":
            assert any(b.block_id == g.right_block and b.genome == g.genome and b.contig == g.contig and b.start == g.end for b in blocks)
    if case == "celegans-A-with-absent-B":
        absent = [g for g in got_gaps if g.genome == "celegans-chrII-III.B.fa"]
        assert [g.kind for g in absent] == ["unplaced", "unplaced"] and sum(g.end - g.start for g in absent) == 15279466 + 13777084


def test_both_files_are_formatted_as_stated():
    occ = 0.25
    rows = [dict(genome="a", contig="c", start=0, end=100, kind="leading", left_block=".", right_block="1", n_bases=100, kmers=0, shared_kmers=0),
            dict(genome="a", contig="c", start=300, end=1300, kind="between", left_block="1", right_block="x2", n_bases=3, kmers=900, shared_kmers=90),
            dict(genome="a", contig="c", start=2000, end=2400, kind="trailing", left_block="x2", right_block=".", n_bases=0, kmers=300, shared_kmers=200)]
    text = gaps.table(rows, 24, 8000, occ)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == ""
    assert lines[0] == "genome\tcontig\tstart\tend\tlength\tkind\tleft_block\tright_block\tn_bases\tkmers\tshared_kmers\tshared_fraction\texcess"
    assert lines[1] == "a\tc\t0\t100\t100\tleading\t.\t1\t100\t0\t0\tNA\tNA"
    assert lines[2] == "a\tc\t300\t1300\t1000\tbetween\t1\tx2\t3\t900\t90\t0.1\t0"                      # below the occupancy: clipped at 0
    assert lines[3] == "a\tc\t2000\t2400\t400\ttrailing\tx2\t.\t0\t300\t200\t0.666667\t0.555556"       # (2/3 - 1/4) / (3/4) = 5/9
    assert lines[4] == "# k 24, filter 8000 bits, occupancy 0.25" and len(lines) == 6
    block_rows = [dict(genome="a", contig="c", start=100, end=300, n_bases=0, kmers=177, shared_kmers=177),
                  dict(genome="b", contig="d", start=0, end=50, n_bases=50, kmers=0, shared_kmers=0)]
    text = gaps.summary(rows, block_rows, 24, 8000, occ, genomes=["b", "a", "never"])
    lines = text.split("\n")
    assert lines[0] == "genome\tpart\tintervals\tbases\tn_bases\tkmers\tshared_kmers\tshared_fraction\texcess"
    assert lines[1] == "a\tin_blocks\t1\t200\t0\t177\t177\t1\t1"
    assert lines[2] == f"a\toutside\t3\t1500\t103\t1200\t290\t{290 / 1200:.6g}\t0"
    assert lines[3] == "b\tin_blocks\t1\t50\t50\t0\t0\tNA\tNA"
    assert lines[4] == "b\toutside\t0\t0\t0\t0\t0\tNA\tNA"
    assert lines[5] == "never\tin_blocks\t0\t0\t0\t0\t0\tNA\tNA" and lines[6] == "never\toutside\t0\t0\t0\t0\t0\tNA\tNA"
    assert lines[7] == "# k 24, filter 8000 bits, occupancy 0.25" and lines[8] == "" and len(lines) == 9
    assert gaps.excess(5, 10, 1.0) == 0.0 and gaps.excess(0, 0, 0.5) is None and gaps.excess(10, 10, 0.5) == 1.0


def test_the_host_half_needs_neither_numpy_nor_torch_nor_the_library():
    import subprocess
    import sys
    code = ("import sys\n"
            "for m in ('numpy', 'torch', 'ctypes'):\n"
            "    sys.modules[m] = None\n"
            "from ntsynt_amd import gaps\n"
            "from ntsynt_amd.assess import BlockRow\n"
            "g, m = gaps.cut([BlockRow('1', 'a', 'c', 5, 9, '+', '', '')], {'a': [('c', 12)]})\n"
            "print(len(g), len(m), gaps.table([], 24, 64, 0.5).count('\\n'))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.split() == ["2", "1", "2"], r.stderr[-2000:]

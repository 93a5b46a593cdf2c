"""The host side of the block lift (ntsynt_amd/assess.py read_bed, lift_queries, lift_rows; docs/design/04_23_block_lift.md) without a GPU:
read_bed and its refusals; lift_queries and lift_rows on hand-made chains -- the source on line a and on line b, `+` and `-` pairs,
clipping at either end, an interval over two chains of one pair, an interval in no chain, 1-base intervals at a chain's first and last
base, an interval inside a run the other genome does not have (it lifts to length 0) -- with tests/lift_brute.py standing in for
nts_cigar_lift, against hand-stated coordinates and against lift_brute.lift_from_paf, which walks the same records base by base; and
the brute force against itself with the sides swapped."""
import numpy as np
import pytest

from ntsynt_amd import assess
from tests import lift_brute as LB

# two pairs of genome A (target) and genome B (query): a `+` pair with two chains and a `-` pair with two chains
#   `5=1X3I2D4=`: 12 bases of A, 13 of B;  `3D2I6=`: 9 of A, 8 of B;  `4=2I`: 4 of A, 6 of B
RECORDS = (("q1", 200, 213, "+", "t1", 100, 112, 0, "5=1X3I2D4=", "7"), ("q1", 250, 258, "+", "t1", 150, 159, 1, "3D2I6=", "7"),
           ("q2", 587, 600, "-", "t2", 1000, 1012, 0, "5=1X3I2D4=", "9"), ("q2", 560, 566, "-", "t2", 1050, 1054, 1, "4=2I", "9"))
PAF = "".join("\t".join(str(v) for v in (q, 5000, q0, q1, sign, t, 6000, t0, t1, 0, 0, 255, "NM:i:0", f"bi:i:{block}", "tg:Z:A", "qg:Z:B", f"ch:i:{ch}",
                                         "cg:Z:" + cg)) + "\n" for q, q0, q1, sign, t, t0, t1, ch, cg, block in RECORDS)


def spans_of(source):
    "lift_queries' spans of RECORDS for the source genome A (line a) or B (line b), and per chain its entries"
    side = 0 if source == "A" else 1
    s = {"pair": [], "chain": [], "side": [], "flip": [], "contig": [], "s0": [], "s1": [], "o0": [], "o1": []}
    for c, (q, q0, q1, sign, t, t0, t1, _, _, block) in enumerate(RECORDS):
        mine, other = ((q, q0, q1), (t, t0, t1)) if side else ((t, t0, t1), (q, q0, q1))
        for f, v in (("pair", int(block)), ("chain", c), ("side", side), ("flip", sign == "-"), ("contig", mine[0]), ("s0", mine[1]), ("s1", mine[2]),
                     ("o0", other[1]), ("o1", other[2])):
            s[f].append(v)
    return {f: (v if f == "contig" else np.array(v)) for f, v in s.items()}


def brute_hits(queries):
    "what nts_cigar_lift returns for these queries, from the column walk"
    from ntsynt_amd.device import LIFT_HIT_DTYPE
    walkers = [LB.Walker(LB.parse_cigar(r[8])) for r in RECORDS]
    hits = np.zeros(queries.size, dtype=LIFT_HIT_DTYPE)
    for n, q in enumerate(queries):
        hits[n] = walkers[int(q["chain"])].lift(int(q["side"]), int(q["pos"])) + (0,)
    return hits


def lifted(source, bed):
    "[(interval, chain, src_start, src_end, to_start, to_end)] through lift_queries and lift_rows, in the order of (interval, chain)"
    intervals = {"contig": [b[0] for b in bed], "name": [b[3] for b in bed], "start": np.array([b[1] for b in bed], dtype=np.int64),
                 "end": np.array([b[2] for b in bed], dtype=np.int64)}
    spans = spans_of(source)
    queries, overlaps = assess.lift_queries(spans, intervals)
    assert queries.size == 2 * overlaps["interval"].size
    rows = assess.lift_rows(spans, overlaps, brute_hits(queries))
    return sorted(zip(*(rows[f].tolist() for f in ("interval", "span", "lo", "hi", "to_start", "to_end"))))


def test_read_bed(tmp_path):
    path = tmp_path / "a.bed"
    path.write_text("# a comment\ntrack name=x\nbrowser position chr1:1-2\n\nchr1\t5\t9\tgene1\t0\t+\nchr2\t0\t1\nchr1 7 8 spaced\n")
    bed = assess.read_bed(str(path))
    assert bed["contig"] == ["chr1", "chr2", "chr1"] and bed["name"] == ["gene1", ".", "spaced"]
    assert bed["start"].tolist() == [5, 0, 7] and bed["end"].tolist() == [9, 1, 8] and bed["start"].dtype == np.int64
    for text, words in (("chr1\t5\t9\nchr1\t9\t9\n", ("line 2", "9")), ("chr1\t5\n", ("line 1", "3 columns")), ("#x\nchr1\t-1\t4\n", ("line 2", "negative")),
                        ("chr1\t8\t3\n", ("line 1",)), ("chr1\ta\t3\n", ("line 1", "integers"))):
        path.write_text(text)
        with pytest.raises(ValueError) as err:
            assess.read_bed(str(path))
        assert all(w in str(err.value) for w in words), (text, str(err.value))
    path.write_text("")
    assert assess.read_bed(str(path))["contig"] == []


def test_the_source_on_line_a():
    bed = [("t1", 102, 105, "inside"), ("t1", 106, 108, "in the 2D run"), ("t1", 90, 103, "clipped at the left"), ("t1", 110, 130, "clipped at the right"),
           ("t1", 105, 155, "two chains"), ("t1", 120, 140, "between the chains"), ("t1", 100, 101, "first base"), ("t1", 111, 112, "last base"),
           ("t1", 150, 151, "first base of a 3D"), ("t2", 1000, 1005, "minus"), ("t2", 1052, 1060, "minus, its insertion behind"), ("t3", 5, 6, "no chain here")]
    got = lifted("A", bed)
    assert got == [(0, 0, 102, 105, 202, 205), (1, 0, 106, 108, 209, 209), (2, 0, 100, 103, 200, 203), (3, 0, 110, 112, 211, 213),
                   (4, 0, 105, 112, 205, 213), (4, 1, 150, 155, 250, 254), (6, 0, 100, 101, 200, 201), (7, 0, 111, 112, 212, 213),
                   (8, 1, 150, 151, 250, 250), (9, 2, 1000, 1005, 595, 600), (10, 3, 1052, 1054, 562, 564)]


def test_the_source_on_line_b():
    bed = [("q1", 206, 209, "in the 3I run"), ("q1", 205, 210, "X to ="), ("q1", 190, 300, "both chains, clipped"), ("q2", 590, 595, "minus"),
           ("q2", 599, 600, "minus: the chain's first base"), ("q2", 587, 588, "minus: its last base"), ("q2", 560, 562, "minus: in the 2I run"),
           ("q2", 500, 700, "minus: both chains")]
    got = lifted("B", bed)
    assert got == [(0, 0, 206, 209, 106, 106), (1, 0, 205, 210, 105, 109), (2, 0, 200, 213, 100, 112), (2, 1, 250, 258, 153, 159), (3, 2, 590, 595, 1005, 1009),
                   (4, 2, 599, 600, 1000, 1001), (5, 2, 587, 588, 1011, 1012), (6, 3, 560, 562, 1054, 1054), (7, 2, 587, 600, 1000, 1012),
                   (7, 3, 560, 566, 1050, 1054)]


@pytest.mark.parametrize("source", ["A", "B"])
def test_lift_rows_against_the_walk_over_the_paf(source):
    "every interval of 1 .. 4 bases around the chains, and a few long ones: the same lines as lift_from_paf makes from the PAF text"
    contigs = {"A": (("t1", 95, 165), ("t2", 995, 1060)), "B": (("q1", 195, 262), ("q2", 555, 605))}[source]
    bed = [(c, s, s + n, f"{c}:{s}+{n}") for c, lo, hi in contigs for s in range(lo, hi) for n in (1, 2, 3, 4)] + \
        [(c, lo, hi, "all") for c, lo, hi in contigs] + [("elsewhere", 1, 2, ".")]
    want, _ = LB.lift_from_paf(PAF, bed, source)
    info = {c: (r[9], "B" if source == "A" else "A", r[0] if source == "A" else r[4], r[3], r[7]) for c, r in enumerate(RECORDS)}
    got, seen = [], set()
    for j, c, lo, hi, to_start, to_end in lifted(source, bed):
        block, other, to_contig, sign, ch = info[c]
        seen.add(j)
        got.append((j, "\t".join(str(v) for v in (source,) + bed[j] + (block, other, to_contig, to_start, to_end, sign, ch, lo, hi,
                                                                         "full" if (lo, hi) == bed[j][1:3] else "partial"))))
    got += [(j, "\t".join(str(v) for v in (source,) + b + (".",) * 9 + ("unmapped",))) for j, b in enumerate(bed) if j not in seen]
    assert [line for _, line in sorted(got, key=lambda g: g[0])] == want
    assert sum("unmapped" in w for w in want) > 10 and sum("partial" in w for w in want) > 10
    assert any(w.split("\t")[8] == w.split("\t")[9] and w.split("\t")[14] == "full" for w in want)        # (a lift to length 0)


def test_chains_out_of_order_are_refused():
    spans = spans_of("A")
    spans["s0"][1], spans["s1"][1] = 105, 120                 # overlaps chain 0 of its pair
    with pytest.raises(ValueError, match="overlap"):
        assess.lift_queries(spans, {"contig": ["t1"], "name": ["."], "start": np.array([100]), "end": np.array([110])})


def test_lift_table_lists_every_line_and_the_parameters():
    rows = [dict(zip(assess.LIFT_COLUMNS, ("A", "t1", 1, 2, "n", "7", "B", "q1", 3, 4, "+", 0, 1, 2, "full"))),
            dict(zip(assess.LIFT_COLUMNS, ("A", "t1", 5, 6, ".") + (".",) * 9 + ("unmapped",)))]
    text = assess.lift_table(rows, 21, 16, 31, 4096, 1023, (1500, 255, 6))
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.LIFT_COLUMNS) and len(assess.LIFT_COLUMNS) == 15
    assert lines[1] == "A\tt1\t1\t2\tn\t7\tB\tq1\t3\t4\t+\t0\t1\t2\tfull" and lines[2].endswith("\t.\tunmapped")
    assert lines[3] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500, ends_max_edits 255, ends_penalty 6"
    assert assess.lift_table([], 21, 16, 31, 4096).splitlines()[1] == "# k 21, rate 16, band 31, max_len 4096, max_edits 0"


def test_the_brute_force_agrees_with_itself_under_swapping_sides():
    rng = np.random.default_rng(3)
    for text in ("5=1X3I2D4=", "3D2I6=", "4=2I", "1=", "3=3="):
        entries = LB.parse_cigar(text)
        swapped = LB.swap_sides(entries)
        cols, len_a, len_b = LB.columns(entries)
        assert LB.columns(swapped)[1:] == (len_b, len_a)
        for side, length in ((0, len_a), (1, len_b)):
            for pos in range(length + 2):
                here, there = LB.lift(entries, side, pos), LB.lift(swapped, 1 - side, pos)
                other = {1: 2, 2: 1}
                assert (here is None and there is None) or (here[:3] == there[:3] and other.get(here[3], here[3]) == there[3]), (text, side, pos)
    entries = [int(length) << 4 | int(code) for length, code in zip(rng.integers(1, 5, 400), np.array([7, 8, 1, 2])[rng.integers(0, 4, 400)])]
    walker, back = LB.Walker(entries), LB.Walker(LB.swap_sides(entries))
    for pos in range(walker.len_a + 1):
        assert walker.lift(0, pos) == LB.lift(entries, 0, pos)
        hit = walker.lift(0, pos)
        if hit[3] in (7, 8):                                  # an aligned base: there and back again, on the swapped chain too
            assert walker.lift(1, hit[0])[0] == pos and back.lift(0, hit[0])[0] == pos

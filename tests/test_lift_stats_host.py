"""The host side of the lift identity (ntsynt_amd/assess.py window_intervals, lift_ranges, lift_identity_table, the switches of ntSynt and
ntsynt_block_stats; docs/design/04_25_lift_identity.md) without a GPU: the brute force tests/lift_stats_brute.py against hand-counted
ranges (ranges that start or end inside the I, the D and the X of `5=1X3I2D4=`, neighbouring entries of one kind), against itself with
the sides swapped, and over windows that tile a chain; window_intervals; the join with the brute force standing in for
nts_cigar_lift_stats; the table; every new parser error and the --dry-run lines."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from tests import lift_brute as LB
from tests import lift_stats_brute as SB
from tests.test_lift_host import PAF, RECORDS, spans_of

# `5=1X3I2D4=`: columns 0 - 4 `=`, 5 X, 6 - 8 I (B's bases 6 - 8), 9 - 10 D (A's bases 6 - 7), 11 - 14 `=`; A = 12 bases, B = 13
#   (side, lo, hi): (oth_lo, oth_hi, eq, x, src_gap, oth_gap, src_gaps, oth_gaps), counted by hand
BY_HAND = {
    "5=1X3I2D4=": {(0, 0, 12): (0, 13, 9, 1, 2, 3, 1, 1), (0, 7, 9): (9, 10, 1, 0, 1, 0, 1, 0), (0, 4, 7): (4, 9, 1, 1, 1, 3, 1, 1),
                   (0, 5, 6): (5, 6, 0, 1, 0, 0, 0, 0), (0, 5, 7): (5, 9, 0, 1, 1, 3, 1, 1), (0, 6, 8): (9, 9, 0, 0, 2, 0, 1, 0),
                   (0, 0, 6): (0, 6, 5, 1, 0, 0, 0, 0),                                     # (the I behind the X lies behind c_hi: not counted)
                   (1, 0, 13): (0, 12, 9, 1, 3, 2, 1, 1), (1, 7, 10): (6, 9, 1, 0, 2, 2, 1, 1), (1, 5, 8): (5, 6, 0, 1, 2, 0, 1, 0),
                   (1, 6, 9): (6, 6, 0, 0, 3, 0, 1, 0),                                     # (the D behind the I lies behind c_hi: not counted)
                   (1, 8, 10): (6, 9, 1, 0, 1, 2, 1, 1), (1, 9, 10): (8, 9, 1, 0, 0, 0, 0, 0)},
    "2=2D2D1X": {(0, 3, 5): (2, 2, 0, 0, 2, 0, 1, 0), (0, 0, 7): (0, 3, 2, 1, 4, 0, 1, 0), (1, 1, 3): (1, 7, 1, 1, 0, 4, 0, 1)},
    "1=2I2I3=": {(0, 0, 2): (0, 6, 2, 0, 0, 4, 0, 1), (1, 2, 4): (1, 1, 0, 0, 2, 0, 1, 0), (1, 0, 8): (0, 4, 4, 0, 4, 0, 1, 0)},
    "3D2I6=": {(0, 0, 3): (0, 0, 0, 0, 3, 0, 1, 0), (0, 2, 4): (0, 3, 1, 0, 1, 2, 1, 1), (1, 0, 2): (3, 3, 0, 0, 2, 0, 1, 0), (1, 0, 3): (3, 4, 1, 0, 2, 0, 1, 0)},
    "1=": {(0, 0, 1): (0, 1, 1, 0, 0, 0, 0, 0), (1, 0, 1): (0, 1, 1, 0, 0, 0, 0, 0)},
}


def test_the_brute_force_against_hand_counted_ranges():
    for text, cases in BY_HAND.items():
        for (side, lo, hi), want in cases.items():
            got = SB.range_stats(LB.parse_cigar(text), side, lo, hi)
            assert got == want, (text, side, lo, hi, got, want)
            assert got[2] + got[3] + got[4] == hi - lo and got[2] + got[3] + got[5] == got[1] - got[0]
    entries = LB.parse_cigar("5=1X3I2D4=")
    for side, lo, hi in ((0, 3, 3), (0, 4, 3), (0, 0, 13), (1, 0, 14), (2, 0, 1), (0, 12, 13)):
        assert SB.range_stats(entries, side, lo, hi) is None


def every_range(entries):
    _, len_a, len_b = LB.columns(entries)
    return [(side, lo, hi) for side, n in ((0, len_a), (1, len_b)) for lo in range(n) for hi in range(lo + 1, n + 1)]


def test_swapping_the_sides_exchanges_the_gap_roles_and_nothing_else():
    for text in ("5=1X3I2D4=", "3D2I6=", "4=2I", "3=3=", "2=2D2D1X", "1=2I2I3="):
        entries = LB.parse_cigar(text)
        here, there = SB.Counter(entries), SB.Counter(LB.swap_sides(entries))
        for side, lo, hi in every_range(entries):
            assert here.stats(side, lo, hi) == there.stats(1 - side, lo, hi), (text, side, lo, hi)


def test_windows_that_tile_a_chain_add_up_to_its_totals():
    rng = np.random.default_rng(3)
    entries = ((rng.integers(1, 6, 400) << 4) | np.array([7, 8, 1, 2])[rng.integers(0, 4, 400)]).tolist()
    counter = SB.Counter(entries)
    total = {code: sum(v >> 4 for v in entries if v & 15 == code) for code in (1, 2, 7, 8)}
    for side, n, src_only, oth_only in ((0, counter.len_a, 2, 1), (1, counter.len_b, 1, 2)):
        for width in (1, 7, 100, n, n + 5):
            rows = [counter.stats(side, lo, min(lo + width, n)) for lo in range(0, n, width)]
            assert sum(r[2] for r in rows) == total[7] and sum(r[3] for r in rows) == total[8] and sum(r[4] for r in rows) == total[src_only]
            assert sum(r[5] for r in rows) <= total[oth_only]                               # (a gap of the other side between two windows is in neither)
            assert all(behind[0] >= front[1] for front, behind in zip(rows[:-1], rows[1:]))  # (the lifted spans do not overlap)
        assert counter.stats(side, 0, n)[5] <= total[oth_only]
        assert sum(r[5] for r in [counter.stats(side, lo, lo + 1) for lo in range(n)]) == 0  # (one base: one column)


def test_window_intervals():
    got = assess.window_intervals([("chr1", 2500), ("chr2", 300), ("chr3", 2000), ("empty", 0)], 1000)
    assert got["contig"] == ["chr1"] * 3 + ["chr2"] + ["chr3"] * 2 and got["name"] == ["w0", "w1", "w2", "w0", "w0", "w1"]
    assert got["start"].tolist() == [0, 1000, 2000, 0, 0, 1000] and got["end"].tolist() == [1000, 2000, 2500, 300, 1000, 2000]
    assert got["start"].dtype == np.int64 and got["end"].dtype == np.int64 and np.all(got["start"] < got["end"])
    assert assess.window_intervals({"a": 5}, 1)["end"].tolist() == [1, 2, 3, 4, 5]
    none = assess.window_intervals([], 10)
    assert none["contig"] == [] and none["start"].size == 0
    for width in (0, -3):
        with pytest.raises(ValueError, match="at least one base"):
            assess.window_intervals([("chr1", 10)], width)


def brute_stats(ranges):
    "what nts_cigar_lift_stats returns for these ranges of RECORDS' chains, from the column walk"
    from ntsynt_amd.device import LIFT_STATS_DTYPE
    counters = [SB.Counter(LB.parse_cigar(r[8])) for r in RECORDS]
    out = np.zeros(ranges.size, dtype=LIFT_STATS_DTYPE)
    for n, r in enumerate(ranges):
        out[n] = counters[int(r["chain"])].stats(int(r["side"]), int(r["lo"]), int(r["hi"])) + (0,)
    return out


@pytest.mark.parametrize("source", ["A", "B"])
def test_lift_ranges_against_the_walk_over_the_paf(source):
    "lift_queries -> lift_ranges -> (the brute force for the device) -> the lifted span of lift_rows and the counts of identity_from_paf"
    from ntsynt_amd.device import LIFT_RANGE_DTYPE
    contigs = {"A": ("t1", "t2"), "B": ("q1", "q2")}[source]
    bed = [(c, s, s + n, f"i{s}_{n}") for c in contigs for s in range(90 if source == "A" else 190, 1100, 7) for n in (1, 4, 30)]
    intervals = {"contig": [b[0] for b in bed], "name": [b[3] for b in bed], "start": np.array([b[1] for b in bed], dtype=np.int64),
                 "end": np.array([b[2] for b in bed], dtype=np.int64)}
    spans = spans_of(source)
    queries, overlaps = assess.lift_queries(spans, intervals)
    ranges, which = assess.lift_ranges(queries, overlaps)
    assert ranges.dtype == LIFT_RANGE_DTYPE and ranges.size == overlaps["interval"].size > 20 and which.tolist() == list(range(ranges.size))
    assert np.all(ranges["lo"] < ranges["hi"]) and (ranges["hi"] - ranges["lo"]).tolist() == (overlaps["hi"] - overlaps["lo"]).tolist()
    stats = brute_stats(ranges)
    want = [ln.split("\t") for ln in SB.identity_from_paf(PAF, bed, source) if not ln.endswith("unmapped")]
    col = {c: i for i, c in enumerate(assess.LIFT_IDENTITY_COLUMNS)}
    # the same overlaps in the same order: per interval the chains in RECORDS' order
    order = np.lexsort((overlaps["span"], overlaps["interval"]))
    assert len(want) == order.size
    for o, w in zip(order.tolist(), want):
        assert [int(stats[f][o]) for f in assess.LIFT_STATS_FIELDS] == [int(w[col[c]]) for c in assess.LIFT_IDENTITY_COLUMNS[14:20]], (o, w)
        assert (int(overlaps["lo"][o]), int(overlaps["hi"][o])) == (int(w[col["src_start"]]), int(w[col["src_end"]]))
        assert int(stats["oth_hi"][o]) - int(stats["oth_lo"][o]) == int(w[col["to_end"]]) - int(w[col["to_start"]])
    wanted = np.zeros(len(bed), dtype=bool)
    wanted[::3] = True
    some, which = assess.lift_ranges(queries, overlaps, wanted)
    assert which.tolist() == np.flatnonzero(wanted[overlaps["interval"]]).tolist() and some.tobytes() == ranges[which].tobytes() and 0 < some.size < ranges.size
    with pytest.raises(ValueError, match="two queries per overlap"):
        assess.lift_ranges(queries[:-1], overlaps)


def test_the_table_its_header_the_unmapped_line_and_the_identity_text():
    assert assess.LIFT_IDENTITY_COLUMNS[:14] == assess.LIFT_COLUMNS[:14] and assess.LIFT_IDENTITY_COLUMNS[-1] == "status"
    assert assess.LIFT_IDENTITY_COLUMNS[14:] == ("matches", "mismatches", "src_gap_bases", "to_gap_bases", "src_gaps", "to_gaps", "columns", "identity", "status")
    bed = [("t1", 95, 130, "across"), ("t1", 400, 410, "nowhere"), ("t1", 106, 108, "deleted"), ("t1", 100, 105, "equal")]
    body = SB.identity_from_paf(PAF, bed, "A")
    rows = [dict(zip(assess.LIFT_IDENTITY_COLUMNS, ln.split("\t"))) for ln in body]
    text = assess.lift_identity_table(rows, 21, 16, 31, 4096, 1023, ends=(1500, 255, 6))
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.LIFT_IDENTITY_COLUMNS) and lines[1:-1] == body
    assert lines[-1] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500, ends_max_edits 255, ends_penalty 6"
    assert assess.lift_identity_table([], 21, 16, 31, 4096).splitlines()[-1] == "# k 21, rate 16, band 31, max_len 4096, max_edits 0"
    by_name = {r["name"]: r for r in rows}
    assert body[1] == "A\tt1\t400\t410\tnowhere" + "\t." * 17 + "\tunmapped"
    assert (by_name["deleted"]["matches"], by_name["deleted"]["columns"], by_name["deleted"]["identity"]) == ("0", "2", "0.000000")
    assert (by_name["equal"]["matches"], by_name["equal"]["columns"], by_name["equal"]["identity"]) == ("5", "5", "1.000000")
    assert (by_name["across"]["status"], by_name["across"]["matches"], by_name["across"]["columns"], by_name["across"]["identity"]) == ("partial", "9", "15", "0.600000")
    assert SB.identity_text(1, 3) == "0.333333" and SB.identity_text(2, 3) == "0.666666"


class FakeGenome:
    def __init__(self, names, rec_len):
        self.names, self.rec_len, self.freed = names, np.array(rec_len, dtype=np.uint64), 0

    def free(self):
        self.freed += 1


def test_record_sizes_reads_a_resident_genome_and_frees_one_it_loaded():
    g = FakeGenome(["chr1", "chr2"], [10, 20])
    assert assess.record_sizes({"x.fa": g}, "x.fa") == [("chr1", 10), ("chr2", 20)] and g.freed == 0
    assert assess.record_sizes({"x.fa": lambda: g}, "x.fa") == [("chr1", 10), ("chr2", 20)] and g.freed == 1
    with pytest.raises(ValueError, match="not among the genomes"):
        assess.record_sizes({"x.fa": g}, "y.fa")


@pytest.fixture()
def fastas(tmp_path):
    paths = []
    for name in ("one.fa", "two.fa"):
        (tmp_path / name).write_text(">chr1\nACGT\n")
        paths.append(str(tmp_path / name))
    return paths


def stopped(argv, capsys, monkeypatch, **env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    with pytest.raises(SystemExit) as stop:
        cli.main(argv)
    assert stop.value.code == 2
    return capsys.readouterr().err


def test_the_parser_errors_of_ntsynt(fastas, capsys, monkeypatch):
    base = fastas + ["-d", "1"]
    assert "--lift-identity counts the alignment columns of the intervals of --block-lift BED" in stopped(base + ["--lift-identity"], capsys, monkeypatch)
    assert "--lift-windows W needs --lift-genome NAME" in stopped(base + ["--lift-windows", "1000"], capsys, monkeypatch)
    assert "a window has at least one base" in stopped(base + ["--lift-windows", "0", "--lift-genome", "one.fa"], capsys, monkeypatch)
    assert "three.fa is not among the genomes" in stopped(base + ["--lift-windows", "10", "--lift-genome", "three.fa"], capsys, monkeypatch)
    assert "--identity-band must lie in 1..31" in stopped(base + ["--lift-windows", "10", "--lift-genome", "one.fa", "--identity-band", "99"], capsys, monkeypatch)
    # --lift-genome with neither switch: the message it always had
    assert "--lift-genome names the genome of the intervals of --block-lift BED" in stopped(base + ["--lift-genome", "one.fa"], capsys, monkeypatch)
    assert "--block-lift BED needs --lift-genome NAME" in stopped(base + ["--block-lift", "x.bed", "--lift-identity"], capsys, monkeypatch)
    err = stopped(base + ["--block-lift", "x.bed", "--lift-genome", "one.fa", "--lift-identity"], capsys, monkeypatch, WORLD_SIZE="2", RANK="0")
    assert "--lift-identity works from the genomes resident on one GPU" in err and "ntsynt_block_stats --tsv" in err and "--lift-identity-out" in err
    err = stopped(base + ["--lift-windows", "10", "--lift-genome", "one.fa"], capsys, monkeypatch, WORLD_SIZE="2", RANK="0")
    assert "--lift-windows works from the genomes resident on one GPU" in err and "ntsynt_block_stats --tsv" in err and "--lift-windows-out" in err


def test_the_dry_run_lists_the_stages_behind_block_lift(fastas, capsys):
    base = fastas + ["-d", "1", "--dry-run"]
    assert cli.main(base + ["--block-lift", "x.bed", "--lift-genome", "one.fa", "--lift-identity", "--lift-windows", "1000", "--block-ends", "--gaps"]) == 0
    out = capsys.readouterr().out
    tail = "k 21, rate 16, band 31, max_len 4096, max_edits 0, ends_max_len 4096, ends_max_edits 255, ends_penalty 6)"
    assert f"-> block_lift (lift_scan, lift_search; x.bed on one.fa; {tail} -> block_lift_identity (lift_stats_scan, lift_stats_search; x.bed on one.fa; {tail} -> "\
           f"block_windows (lift_stats_scan, lift_stats_search; windows of 1000 on one.fa; {tail} -> gaps" in out, out
    assert cli.main(base + ["--lift-windows", "500", "--lift-genome", "two.fa"]) == 0
    out = capsys.readouterr().out
    assert out.rstrip().endswith("ntsynt_synteny -> block_windows (lift_stats_scan, lift_stats_search; windows of 500 on two.fa; k 21, rate 16, band 31, "
                                 "max_len 4096, max_edits 0)") and "block_lift" not in out
    assert cli.main(base + ["--block-lift", "x.bed", "--lift-genome", "one.fa"]) == 0
    out = capsys.readouterr().out
    assert "lift_stats" not in out and "block_windows" not in out


def tool_stopped(argv, capsys):
    with pytest.raises(SystemExit) as stop:
        assess.main(["--tsv", "x.tsv", "--fai", "x.fai"] + argv)
    assert stop.value.code == 2
    return capsys.readouterr().err


def test_the_parser_errors_of_the_tool(capsys):
    assert "--lift-identity-out needs the intervals: --lift-bed" in tool_stopped(["--lift-identity-out", "o.tsv", "--lift-genome", "one.fa"], capsys)
    assert "--lift-windows and --lift-windows-out go together" in tool_stopped(["--lift-windows", "10", "--lift-genome", "one.fa"], capsys)
    assert "--lift-windows and --lift-windows-out go together" in tool_stopped(["--lift-windows-out", "o.tsv", "--lift-genome", "one.fa"], capsys)
    assert "--lift-windows needs --lift-genome" in tool_stopped(["--lift-windows", "10", "--lift-windows-out", "o.tsv"], capsys)
    assert "at least one base" in tool_stopped(["--lift-windows", "0", "--lift-windows-out", "o.tsv", "--lift-genome", "one.fa"], capsys)
    assert "go together" in tool_stopped(["--lift-bed", "x.bed", "--lift-identity-out", "o.tsv"], capsys)
    assert "go together" in tool_stopped(["--lift-bed", "x.bed", "--lift-genome", "one.fa", "--lift-windows", "10", "--lift-windows-out", "o.tsv"], capsys)
    assert "needs the genomes: --fastas" in tool_stopped(["--lift-windows", "10", "--lift-windows-out", "o.tsv", "--lift-genome", "one.fa"], capsys)
    assert "one.fa is not among the genomes" in tool_stopped(["--lift-bed", "x.bed", "--lift-identity-out", "o.tsv", "--lift-genome", "one.fa", "--fastas", "a.fa"],
                                                             capsys)

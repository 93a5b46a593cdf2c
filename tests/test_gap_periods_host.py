"""The host side of the gap periods (ntsynt_amd/gaps.py period_row, periods_table; the two argument parsers), without a GPU: a gap's line
from the device's five numbers, driven by hand at the edges of its classes and of the copy count's rounding, and where the switch and
the tool's option are accepted and refused.  docs/design/04_14_gap_periods.md."""
import pytest

from ntsynt_amd import cli, gaps
from tests.periods_brute import brute_line

GAP = {"genome": "g1.fa", "contig": "chr1", "start": 1000, "end": 3000, "kind": "between", "left_block": "3", "right_block": "4"}


def _row(result, k=24, sampled=50, min_hits=4, gap=GAP):
    row = gaps.period_row(gap, k, sampled, result, min_hits)
    assert set(row) == set(gaps.PERIOD_COLUMNS)
    line = ["." if row[c] is None else str(row[c]) for c in gaps.PERIOD_COLUMNS]
    assert line[:6] == [gap["genome"], gap["contig"], str(gap["start"]), str(gap["end"]), str(gap["end"] - gap["start"]), gap["kind"]]
    assert line[6:] == brute_line((gap["genome"], gap["contig"], gap["start"], gap["end"], gap["kind"]), k, sampled, result, min_hits)
    return row


def test_below_min_hits_the_line_is_dots():
    row = _row((9, 171, 3, 5, 900))
    assert (row["sampled"], row["recurring"], row["period_hits"], row["class"]) == (50, 9, 3, ".")
    assert [row[c] for c in ("period", "from", "to", "copies", "covered_fraction")] == [None] * 5
    assert _row((9, 171, 4, 5, 900))["class"] != "."                                # at min_hits: a line
    assert _row((0, 0, 0, 0, 0))["class"] == "." and _row((0, 0, 0, 0, 0), sampled=0)["sampled"] == 0
    assert _row((1, 7, 1, 0, 7), min_hits=1)["period"] == 7


def test_tandem_against_partial_at_half_the_gap():
    # length 2000, k 24: covered = last_off + 24 - first_off
    half = _row((30, 100, 10, 10, 986))                                             # covered 1000: 2 * covered == length
    assert (half["from"], half["to"], half["class"], half["covered_fraction"]) == (1010, 2010, "partial", "0.5")
    more = _row((30, 100, 10, 10, 987))                                             # one base beyond
    assert (more["from"], more["to"], more["class"], more["covered_fraction"]) == (1010, 2011, "tandem", "0.5005")
    whole = _row((30, 100, 10, 0, 1976))
    assert (whole["from"], whole["to"], whole["class"], whole["covered_fraction"]) == (1000, 3000, "tandem", "1")


def test_copies_are_tenths_rounded_down():
    wide = dict(GAP, end=20_000)
    # period 171, k 24: covered = last_off + 24
    assert _row((99, 171, 40, 0, 6839 - 24), gap=wide)["copies"] == "39.9"          # 6839 = 40 * 171 - 1
    assert _row((99, 171, 40, 0, 6840 - 24), gap=wide)["copies"] == "40.0"
    assert _row((99, 171, 40, 0, 6822 - 24), gap=wide)["copies"] == "39.8"          # 39.89...: down, not to the nearest
    assert _row((5, 500, 4, 0, 1000 - 24))["copies"] == "2.0"
    assert _row((5, 500, 4, 100, 100 + 1000 - 24))["copies"] == "2.0"               # from first_off, not from the gap's start


def test_the_table_its_columns_and_its_footer():
    assert gaps.PERIOD_COLUMNS == ("genome", "contig", "start", "end", "length", "kind", "sampled", "recurring", "period", "period_hits", "from", "to",
                                   "copies", "covered_fraction", "class")
    rows = [_row((30, 100, 10, 10, 987)), _row((2, 9, 2, 0, 9))]
    text = gaps.periods_table(rows, 24, 16, 4)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 5
    assert lines[0] == "\t".join(gaps.PERIOD_COLUMNS)
    assert lines[1] == "g1.fa\tchr1\t1000\t3000\t2000\tbetween\t50\t30\t100\t10\t1010\t2011\t10.0\t0.5005\ttandem"
    assert lines[2] == "g1.fa\tchr1\t1000\t3000\t2000\tbetween\t50\t2\t.\t2\t.\t.\t.\t.\t."
    assert lines[3] == "# k 24, rate 16, min_hits 4"
    assert gaps.periods_table([], 150, 1, 1) == "\t".join(gaps.PERIOD_COLUMNS) + "\n# k 150, rate 1, min_hits 1\n"


def _fastas(tmp_path):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    return paths


def test_the_switch_implies_gaps_and_is_listed(tmp_path, capsys):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    args = parser.parse_args(paths + ["-d", "1"])
    assert args.gap_periods is False
    cli.check_reports(parser, args)
    assert not args.gap_periods and not args.gaps
    args = parser.parse_args(paths + ["-d", "1", "--gap-periods", "--gap-links-rate", "8", "--gap-links-min", "2"])
    cli.check_reports(parser, args)
    assert args.gap_periods and args.gaps and not args.gap_links and not args.gap_copies and not args.gap_copy_sites
    assert (args.gap_links_rate, args.gap_links_min) == (8, 2)
    assert cli.main(paths + ["-d", "1", "--gap-periods", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_periods")
    assert cli.main(paths + ["-d", "1", "--gap-copy-sites", "--gap-links", "--gap-periods", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_copies -> gap_copy_sites -> gap_periods")
    assert cli.main(paths + ["-d", "1", "--gaps", "-n"]) == 0                       # without the switch: the list it had
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps")
    for bad in (["--gap-links-min", "0"], ["--gap-links-rate", "0"]):
        with pytest.raises(SystemExit):
            cli.main(paths + ["-d", "1", "--gap-periods", "-n"] + bad)


def test_the_switch_is_refused_without_a_filter_and_under_several_ranks(tmp_path, capsys, monkeypatch):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-periods", "--no-common"]))
    assert "--gap-periods reads the common Bloom filter: not with --no-common" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-periods"]))
    err = capsys.readouterr().err
    assert "--gap-periods works from the genomes resident on one GPU" in err and "--periods-out <prefix>.gap_periods.tsv" in err
    monkeypatch.setenv("WORLD_SIZE", "1")
    cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-periods"]))              # one rank: accepted


def test_the_tool_takes_periods_out_with_or_without_the_other_options():
    base = ["--tsv", "g.synteny_blocks.tsv", "--fastas", "a.fa", "b.fa", "--common", "g.common.bf"]
    p = gaps.build_parser()
    assert p.parse_args(base).periods_out is None
    args = p.parse_args(base + ["--periods-out", "p.tsv", "--links-rate", "8"])
    assert (args.periods_out, args.links_rate, args.links_min, args.copies_out, args.links_out) == ("p.tsv", 8, 4, None, None)
    args = p.parse_args(base + ["--links-out", "l.tsv", "--copies-out", "c.tsv", "--copy-sites-out", "s.tsv", "--periods-out", "p.tsv"])
    assert (args.links_out, args.copies_out, args.copy_sites_out, args.periods_out) == ("l.tsv", "c.tsv", "s.tsv", "p.tsv")
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--periods-out"])
    with pytest.raises(SystemExit):
        gaps.main(base + ["--periods-out", "p.tsv", "--links-min", "0"])
    with pytest.raises(FileNotFoundError):                                          # parsed and accepted: main gets as far as its inputs
        gaps.main(["--tsv", "/nonexistent/t.tsv", "--fastas", "/nonexistent/a.fa", "--common", "/nonexistent/c.bf", "--periods-out", "p.tsv"])


def test_periods_refuses_bad_parameters_before_any_device_work():
    for kw in ({"rate": 0}, {"min_hits": 0}):
        with pytest.raises(ValueError, match="periods"):
            gaps.periods(None, {}, 24, [], **kw)
    with pytest.raises(ValueError, match="sample_all"):
        gaps.sample_all({}, 24, [], 0)
    from ntsynt_amd import pipeline
    with pytest.raises(ValueError, match="gap_periods"):
        pipeline.run(["a.fa", "b.fa"], gap_periods=(0, 4), backend=object())

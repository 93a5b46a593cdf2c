"""Gap copies, the host side (ntsynt_amd/gaps.py copy_stats / copies_table, the command lines' switches): no GPU."""
import pytest

from ntsynt_amd import cli, gaps

NA5 = {"absent_some": None, "copies_own_median": None, "copies_own_max": None, "copies_any_median": None, "class": "."}


def test_a_gap_without_sampled_kmers():
    for counts in ([[], [], []], [], [[]]):
        assert gaps.copy_stats(counts, 0) == dict(NA5, sampled=0, single_own=0, single_all=0)


def test_the_lower_median_of_even_and_odd_numbers_of_records():
    odd = gaps.copy_stats([[5, 1, 3], [1, 1, 1]], 0)                             # sorted 1 3 5: the middle one
    assert (odd["sampled"], odd["copies_own_median"], odd["copies_own_max"], odd["copies_any_median"]) == (3, 3, 5, 3)
    even = gaps.copy_stats([[7, 1, 3, 5], [1, 9, 1, 1]], 0)                      # sorted 1 3 5 7: the lower of the two middle ones
    assert (even["sampled"], even["copies_own_median"], even["copies_own_max"]) == (4, 3, 7)
    assert even["copies_any_median"] == 5                                      # the largest count per record: 7 9 3 5 -> 3 5 7 9 -> 5
    assert gaps.copy_stats([[7, 1, 3, 5], [1, 9, 1, 1]], 1)["copies_own_median"] == 1 and gaps.copy_stats([[7, 1, 3, 5], [1, 9, 1, 1]], 1)["copies_own_max"] == 9
    two = gaps.copy_stats([[2, 4]], 0)
    assert (two["copies_own_median"], two["copies_any_median"]) == (2, 2)
    one = gaps.copy_stats([[6]], 0)
    assert (one["copies_own_median"], one["copies_own_max"], one["copies_any_median"], one["class"]) == (6, 6, 6, "repeat")
    assert all(isinstance(v, int) for c, v in even.items() if c != "class")


def test_records_are_counted_not_distinct_hashes():
    "a hash the gap holds twice has two columns, both with the genome-wide count"
    s = gaps.copy_stats([[2, 2, 1], [1, 1, 1]], 0)
    assert (s["sampled"], s["single_own"], s["single_all"], s["copies_own_median"], s["class"]) == (3, 1, 1, 2, "repeat")


def test_the_classes_and_their_boundaries():
    own_of = lambda singles, m: [1] * singles + [2] * (m - singles)               # noqa: E731
    # unique needs MORE than half of the records single everywhere
    assert gaps.copy_stats([own_of(3, 4), [1] * 4], 0)["class"] == "unique"
    half = gaps.copy_stats([own_of(2, 4), [1] * 4], 0)                           # 2 * single_all == m: not unique; 2 * (m - single_own) == m: not repeat
    assert (half["single_own"], half["single_all"], half["class"]) == (2, 2, "mixed")
    assert gaps.copy_stats([own_of(1, 4), [1] * 4], 0)["class"] == "repeat"
    assert gaps.copy_stats([own_of(2, 5), [1] * 5], 0)["class"] == "repeat" and gaps.copy_stats([own_of(3, 5), [1] * 5], 0)["class"] == "unique"
    # single in the own genome but not elsewhere: neither unique nor a repeat of the own genome
    other = gaps.copy_stats([[1] * 4, [1, 3, 3, 3]], 0)
    assert (other["single_own"], other["single_all"], other["class"]) == (4, 1, "mixed")
    assert gaps.copy_stats([[1] * 4, [1, 3, 3, 3]], 1)["class"] == "repeat"     # the same counts seen from the genome that holds them thrice
    # unique comes first: more than half single everywhere decides, whatever the rest is
    assert gaps.copy_stats([[1, 1, 1, 50, 60], [1, 1, 1, 0, 0]], 0)["class"] == "unique"
    assert gaps.copy_stats([[1], [1], [1]], 2)["class"] == "unique" and gaps.copy_stats([[0], [1]], 0)["class"] == "repeat"
    assert gaps.copy_stats([[], []], 1)["class"] == "."


def test_absent_some_counts_records_some_genome_lacks():
    s = gaps.copy_stats([[1, 1, 1, 2, 1], [1, 0, 1, 0, 1], [0, 0, 1, 5, 1]], 0)
    assert (s["absent_some"], s["single_all"], s["single_own"], s["copies_any_median"], s["class"]) == (3, 2, 4, 1, "mixed")
    assert gaps.copy_stats([[1, 2], [3, 4]], 0)["absent_some"] == 0


def _row(**over):
    row = {"genome": "b.fa", "contig": "chr1", "start": 90_000, "end": 96_000, "left_block": "0", "right_block": "1"}
    row.update(gaps.copy_stats([[1] * 10, [2] * 10], 1))
    row.update(over)
    return row


def test_copies_table_formatting():
    assert gaps.COPY_COLUMNS == ("genome", "contig", "start", "end", "left_block", "right_block", "sampled", "single_own", "single_all", "absent_some",
                                 "copies_own_median", "copies_own_max", "copies_any_median", "class")
    empty = dict(_row(start=0, end=12, left_block="."), **gaps.copy_stats([[], []], 1))
    text = gaps.copies_table([_row(), empty], 24, 16, 4194304, 1234, 7, 250)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 5
    assert lines[0].split("\t") == list(gaps.COPY_COLUMNS)
    assert lines[1] == "b.fa\tchr1\t90000\t96000\t0\t1\t10\t0\t0\t0\t2\t2\t2\trepeat"
    assert lines[2] == "b.fa\tchr1\t0\t12\t.\t1\t0\t0\t0\tNA\tNA\tNA\tNA\t."
    assert lines[3] == "# k 24, rate 16, filter 4194304 bits, set 1234 hashes, absent 7 of 250 sampled"
    assert gaps.copies_table([], 150, 1, 64, 0, 0, 0) == "\t".join(gaps.COPY_COLUMNS) + "\n# k 150, rate 1, filter 64 bits, set 0 hashes, absent 0 of 0 sampled\n"


def _fastas(tmp_path):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    return paths


def test_the_switch_implies_gaps_and_shares_the_links_rate(tmp_path, capsys):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    args = parser.parse_args(paths + ["-d", "1"])
    assert args.gap_copies is False                                             # the default
    cli.check_reports(parser, args)
    assert not args.gap_copies and not args.gaps and not args.gap_links and not args.gap_block_links
    args = parser.parse_args(paths + ["-d", "1", "--gap-copies", "--gap-links-rate", "8"])
    assert args.gap_copies and not args.gaps
    cli.check_reports(parser, args)
    assert args.gap_copies and args.gaps and args.gap_links_rate == 8
    assert not args.gap_links and not args.gap_block_links                      # it needs neither link report
    args = parser.parse_args(paths + ["-d", "1", "--gap-block-links"])
    cli.check_reports(parser, args)
    assert args.gap_links and not args.gap_copies                               # and neither of them brings it
    assert cli.main(paths + ["-d", "1", "--gap-copies", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_copies")
    assert cli.main(paths + ["-d", "1", "--gap-copies", "--gap-links", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_copies")
    assert cli.main(paths + ["-d", "1", "--assess", "--gaps", "--gap-links", "--gap-block-links", "--gap-copies", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> assess -> gaps -> gap_links -> gap_block_links -> gap_copies")
    assert cli.main(paths + ["-d", "1", "--gap-block-links", "-n"]) == 0        # without the switch: the list it had
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_block_links")
    with pytest.raises(SystemExit):
        cli.main(paths + ["-d", "1", "--gap-copies", "-n", "--gap-links-rate", "0"])


def test_the_switch_is_refused_without_a_filter_and_under_several_ranks(tmp_path, capsys, monkeypatch):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copies", "--no-common"]))
    assert "--gap-copies reads the common Bloom filter: not with --no-common" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copies"]))
    err = capsys.readouterr().err
    assert "--gap-copies works from the genomes resident on one GPU" in err and "--copies-out <prefix>.gap_copies.tsv" in err
    monkeypatch.setenv("WORLD_SIZE", "1")
    cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copies"]))             # one rank: accepted


def test_the_tool_takes_copies_out_with_or_without_the_link_options():
    base = ["--tsv", "g.synteny_blocks.tsv", "--fastas", "a.fa", "b.fa", "--common", "g.common.bf"]
    p = gaps.build_parser()
    args = p.parse_args(base)
    assert args.copies_out is None and args.links_out is None and args.block_links_out is None and args.links_rate == gaps.LINKS_RATE == 16
    args = p.parse_args(base + ["--copies-out", "c.tsv", "--links-rate", "4"])
    assert args.copies_out == "c.tsv" and args.links_rate == 4 and args.links_out is None and args.block_links_out is None
    args = p.parse_args(base + ["--links-out", "l.tsv", "--block-links-out", "b.tsv", "--copies-out", "c.tsv"])
    assert (args.links_out, args.block_links_out, args.copies_out) == ("l.tsv", "b.tsv", "c.tsv")
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--copies-out"])
    with pytest.raises(FileNotFoundError):                                      # parsed and accepted: main gets as far as its inputs
        gaps.main(["--tsv", "/nonexistent/t.tsv", "--fastas", "/nonexistent/a.fa", "--common", "/nonexistent/c.bf", "--copies-out", "c.tsv"])

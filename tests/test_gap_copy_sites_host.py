"""Gap copy sites, the host side (ntsynt_amd/gaps.py site_placement / site_usable / copy_sites_table, the command lines' switches): no GPU."""
import pytest

from ntsynt_amd import cli, gaps

GAP = {"genome": "b.fa", "contig": "chr1", "start": 1000, "end": 7000, "left_block": "3", "right_block": "4"}


def test_placement_self_own_other():
    assert gaps.site_placement(GAP, "b.fa", "chr1", 1200, 6900) == "self"
    assert gaps.site_placement(GAP, "b.fa", "chr1", 0, 100_000) == "self"         # a site that holds the gap
    assert gaps.site_placement(GAP, "b.fa", "chr2", 1200, 6900) == "own"          # the same numbers on another contig
    assert gaps.site_placement(GAP, "b.fa", "chr1", 50_000, 56_000) == "own"
    assert gaps.site_placement(GAP, "a.fa", "chr1", 1200, 6900) == "other"        # the same place in another genome
    assert gaps.site_placement(GAP, "c.fa", "chr9", 0, 10) == "other"


def test_a_site_that_touches_the_gap_by_one_base_and_one_that_does_not():
    "[from_t, to_t) against [start, end): half-open on both sides"
    assert gaps.site_placement(GAP, "b.fa", "chr1", 6999, 7500) == "self"         # the gap's last base
    assert gaps.site_placement(GAP, "b.fa", "chr1", 7000, 7500) == "own"          # starts where the gap ends
    assert gaps.site_placement(GAP, "b.fa", "chr1", 400, 1001) == "self"          # the gap's first base
    assert gaps.site_placement(GAP, "b.fa", "chr1", 400, 1000) == "own"           # ends where the gap starts


def test_usable_and_over_cap_from_a_count_matrix():
    counts = [[1, 2, 3, 0, 17], [1, 1, 1, 1, 1], [0, 16, 17, 40, 2]]             # three genomes, five records
    assert gaps.site_usable(counts, 16) == ([3, 5, 2], 3)                          # 17 | - | 17, 40
    assert gaps.site_usable(counts, 1) == ([1, 5, 0], 7)                           # 2, 3, 17 | - | 16, 17, 40, 2
    assert gaps.site_usable(counts, 2) == ([2, 5, 1], 5)
    assert gaps.site_usable(counts, (1 << 32) - 1) == ([4, 5, 4], 0)               # a count of 0 is never usable
    assert gaps.site_usable([[], []], 16) == ([0, 0], 0) and gaps.site_usable([], 16) == ([], 0)


def _row(**over):
    row = dict(GAP, **{"class": "repeat", "target_genome": "b.fa", "target_contig": "chr2", "from_t": 20_000, "to_t": 26_010, "blocks": "7,8", "hits": 230,
                       "orientation": "+", "from": 1003, "to": 6990, "sampled": 246, "usable": 240, "placement": "own"})
    row.update(over)
    return row


def test_the_table_its_columns_and_its_footer():
    assert gaps.SITE_COLUMNS == ("genome", "contig", "start", "end", "left_block", "right_block", "class", "target_genome", "target_contig", "from_t", "to_t",
                                 "blocks", "hits", "orientation", "from", "to", "sampled", "usable", "placement")
    text = gaps.copy_sites_table([_row(), _row(target_genome="a.fa", blocks=".", placement="other", orientation="-")], 24, 16, 16, 1000, 4, 4194304, 1234, 9, 750)
    lines = text.splitlines()
    assert text.endswith("\n") and len(lines) == 4
    assert lines[0].split("\t") == list(gaps.SITE_COLUMNS)
    assert lines[1] == "b.fa\tchr1\t1000\t7000\t3\t4\trepeat\tb.fa\tchr2\t20000\t26010\t7,8\t230\t+\t1003\t6990\t246\t240\town"
    assert lines[2].split("\t")[7:] == ["a.fa", "chr2", "20000", "26010", ".", "230", "-", "1003", "6990", "246", "240", "other"]
    assert lines[3] == "# k 24, rate 16, cap 16, step 1000, min_hits 4, filter 4194304 bits, set 1234 hashes, over_cap 9 of 750"
    # no site at all: the header and the footer
    assert gaps.copy_sites_table([], 150, 1, 1, 0, 1, 64, 0, 0, 0) == \
        "\t".join(gaps.SITE_COLUMNS) + "\n# k 150, rate 1, cap 1, step 0, min_hits 1, filter 64 bits, set 0 hashes, over_cap 0 of 0\n"


def _fastas(tmp_path):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    return paths


def test_the_switch_implies_gap_copies_and_shares_rate_and_minimum(tmp_path, capsys):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    args = parser.parse_args(paths + ["-d", "1"])
    assert args.gap_copy_sites is False and args.gap_sites_cap == gaps.SITES_CAP == 16 and args.gap_sites_step == gaps.SITES_STEP == 1000
    cli.check_reports(parser, args)
    assert not args.gap_copy_sites and not args.gap_copies and not args.gaps
    args = parser.parse_args(paths + ["-d", "1", "--gap-copy-sites", "--gap-sites-cap", "3", "--gap-sites-step", "0", "--gap-links-min", "2"])
    cli.check_reports(parser, args)
    assert args.gap_copy_sites and args.gap_copies and args.gaps and not args.gap_links and not args.gap_block_links
    assert (args.gap_sites_cap, args.gap_sites_step, args.gap_links_min, args.gap_links_rate) == (3, 0, 2, 16)
    args = parser.parse_args(paths + ["-d", "1", "--gap-copies"])
    cli.check_reports(parser, args)
    assert args.gap_copies and not args.gap_copy_sites                             # --gap-copies does not bring it
    assert cli.main(paths + ["-d", "1", "--gap-copy-sites", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_copies -> gap_copy_sites")
    assert cli.main(paths + ["-d", "1", "--gap-block-links", "--gap-copy-sites", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_block_links -> gap_copies -> gap_copy_sites")
    assert cli.main(paths + ["-d", "1", "--gap-copies", "-n"]) == 0                # without the switch: the list it had
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_copies")
    for bad in (["--gap-sites-cap", "0"], ["--gap-sites-step", "-1"], ["--gap-links-min", "0"], ["--gap-links-rate", "0"]):
        with pytest.raises(SystemExit):
            cli.main(paths + ["-d", "1", "--gap-copy-sites", "-n"] + bad)


def test_the_switch_is_refused_without_a_filter_and_under_several_ranks(tmp_path, capsys, monkeypatch):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copy-sites", "--no-common"]))
    assert "--gap-copy-sites reads the common Bloom filter: not with --no-common" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copy-sites"]))
    err = capsys.readouterr().err
    assert "--gap-copy-sites works from the genomes resident on one GPU" in err and "--copy-sites-out <prefix>.gap_copy_sites.tsv" in err
    monkeypatch.setenv("WORLD_SIZE", "1")
    cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-copy-sites"]))          # one rank: accepted


def test_the_tool_takes_copy_sites_out_with_or_without_the_other_options():
    base = ["--tsv", "g.synteny_blocks.tsv", "--fastas", "a.fa", "b.fa", "--common", "g.common.bf"]
    p = gaps.build_parser()
    args = p.parse_args(base)
    assert args.copy_sites_out is None and args.sites_cap == 16 and args.sites_step == 1000 and args.copies_out is None
    args = p.parse_args(base + ["--copy-sites-out", "s.tsv", "--sites-cap", "1", "--sites-step", "250"])
    assert (args.copy_sites_out, args.sites_cap, args.sites_step, args.copies_out, args.links_out) == ("s.tsv", 1, 250, None, None)
    args = p.parse_args(base + ["--links-out", "l.tsv", "--block-links-out", "b.tsv", "--copies-out", "c.tsv", "--copy-sites-out", "s.tsv"])
    assert (args.links_out, args.block_links_out, args.copies_out, args.copy_sites_out) == ("l.tsv", "b.tsv", "c.tsv", "s.tsv")
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--copy-sites-out"])
    with pytest.raises(SystemExit):
        gaps.main(base + ["--copy-sites-out", "s.tsv", "--sites-cap", "0"])
    with pytest.raises(FileNotFoundError):                                         # parsed and accepted: main gets as far as its inputs
        gaps.main(["--tsv", "/nonexistent/t.tsv", "--fastas", "/nonexistent/a.fa", "--common", "/nonexistent/c.bf", "--copy-sites-out", "s.tsv"])


def test_copy_sites_refuses_bad_parameters_before_any_device_work():
    for kw in ({"rate": 0}, {"cap": 0}, {"step": -1}, {"min_hits": 0}):
        with pytest.raises(ValueError, match="copy_sites"):
            gaps.copy_sites(None, {}, 24, [], [], [], [], **kw)

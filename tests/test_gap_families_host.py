"""The host side of the gap families (ntsynt_amd/gaps.py family_row, family_site_row, family_site_placement, the two tables; the two
argument parsers), without a GPU: the rows driven by hand, the precedence of the placements, both tables' text with their `.` fields
and their footer, and where the switch and the tool's two options are accepted and refused.  docs/design/04_15_gap_families.md."""
import pytest

from ntsynt_amd import cli, gaps

ARRAY = {"genome": "g1.fa", "contig": "chr1", "start": 1000, "end": 3000, "kind": "between", "left_block": "3", "right_block": "4"}
OTHER = {"genome": "g1.fa", "contig": "chr1", "start": 5000, "end": 6000, "kind": "between", "left_block": "4", "right_block": "5"}
ELSEWHERE = {"genome": "g2.fa", "contig": "chr1", "start": 1000, "end": 3000, "kind": "between", "left_block": "3", "right_block": "4"}
PERIOD_ROW = dict(ARRAY, length=2000, sampled=50, recurring=30, period=100, period_hits=10, to=2011, copies="10.0", covered_fraction="0.5005",
                  **{"from": 1010, "class": "tandem"})


def test_an_arrays_row():
    row = gaps.family_row(PERIOD_ROW, 2, 3, 2, 11, 7)
    assert set(row) == set(gaps.FAMILY_COLUMNS)
    assert [row[c] for c in gaps.FAMILY_COLUMNS] == ["g1.fa", "chr1", 1000, 3000, 2000, "between", 100, "tandem", 2, 3, 2, 11, 7]


def test_placement_by_precedence():
    every = [ARRAY, OTHER, ELSEWHERE]
    place = gaps.family_site_placement
    assert place("g1.fa", "chr1", 2990, 3100, [ARRAY], every) == "array"                        # ten bases into the member array
    assert place("g1.fa", "chr1", 3000, 3100, [ARRAY], every) == "block"                        # [from, to) against [start, end): touching is outside
    assert place("g1.fa", "chr1", 900, 1000, [ARRAY], every) == "block"
    assert place("g1.fa", "chr1", 900, 1001, [ARRAY], every) == "array"
    assert place("g1.fa", "chr1", 5500, 5600, [ARRAY], every) == "gap"                          # a gap that is no member of the family
    assert place("g1.fa", "chr1", 2500, 5500, [ARRAY], every) == "array"                        # both: the array comes first
    assert place("g1.fa", "chr1", 5500, 5600, [ARRAY, OTHER], every) == "array"
    assert place("g1.fa", "chr2", 1500, 1600, [ARRAY], every) == "block"                        # another record
    assert place("g2.fa", "chr1", 1500, 1600, [ARRAY], every) == "gap"                          # another genome's gap, no member
    assert place("g3.fa", "chr1", 1500, 1600, [ARRAY], every) == "block"
    assert place("g1.fa", "chr1", 1500, 1600, [], []) == "block"


def test_a_sites_row_its_copies_and_its_dots():
    row = gaps.family_site_row(1, "g1.fa", "chr2", 150_002, 151_343, 86, 24, 171, 75, 4, ["6"], "block")
    assert set(row) == set(gaps.FAMILY_SITE_COLUMNS)
    assert [row[c] for c in gaps.FAMILY_SITE_COLUMNS] == [1, "g1.fa", "chr2", 150_002, 151_367, 1365, 86, 171, 75, "7.9", "6", "block"]
    # to = last + k; copies = (10 * (to - from)) // period, down: 6839 / 171 = 39.99..., 6840 / 171 = 40
    assert gaps.family_site_row(1, "g", "c", 0, 6839 - 24, 9, 24, 171, 9, 4, [], "array")["copies"] == "39.9"
    assert gaps.family_site_row(1, "g", "c", 0, 6840 - 24, 9, 24, 171, 9, 4, [], "array")["copies"] == "40.0"
    assert gaps.family_site_row(1, "g", "c", 100, 1100 - 24, 9, 24, 500, 4, 4, [], "array")["copies"] == "2.0"     # from `from`, not from 0
    assert gaps.family_site_row(1, "g", "c", 0, 10, 9, 24, 5, 4, 4, ["2", "7"], "gap")["blocks"] == "2,7"
    assert gaps.family_site_row(1, "g", "c", 0, 10, 9, 24, 5, 4, 4, [], "gap")["blocks"] == "."
    below = gaps.family_site_row(3, "g", "c", 0, 10, 9, 24, 5, 3, 4, [], "block")               # period_hits below min_hits
    assert [below[c] for c in ("period", "period_hits", "copies")] == [None] * 3 and (below["hits"], below["length"]) == (9, 34)
    assert gaps.family_site_row(3, "g", "c", 0, 10, 9, 24, 0, 0, 1, [], "block")["period"] is None   # nothing recurs


def test_both_tables_their_columns_and_their_footer():
    assert gaps.FAMILY_COLUMNS == ("genome", "contig", "start", "end", "length", "kind", "period", "class", "family", "members", "genomes",
                                   "array_hashes", "shared_hashes")
    assert gaps.FAMILY_SITE_COLUMNS == ("family", "genome", "contig", "from", "to", "length", "hits", "period", "period_hits", "copies", "blocks",
                                        "placement")
    rows = [gaps.family_row(PERIOD_ROW, 1, 2, 2, 11, 11), gaps.family_row(dict(PERIOD_ROW, genome="g2.fa", **{"class": "partial"}), 1, 2, 2, 9, 9),
            gaps.family_row(dict(PERIOD_ROW, start=7000, end=9000, period=340), 2, 1, 1, 23, 0)]
    text = gaps.families_table(rows, 24, 16, 4, 1000, 34)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 6
    assert lines[0] == "\t".join(gaps.FAMILY_COLUMNS)
    assert lines[1] == "g1.fa\tchr1\t1000\t3000\t2000\tbetween\t100\ttandem\t1\t2\t2\t11\t11"
    assert lines[2] == "g2.fa\tchr1\t1000\t3000\t2000\tbetween\t100\tpartial\t1\t2\t2\t9\t9"
    assert lines[3] == "g1.fa\tchr1\t7000\t9000\t2000\tbetween\t340\ttandem\t2\t1\t1\t23\t0"
    footer = "# k 24, rate 16, min_hits 4, step 1000, arrays 3, families 2, set 34 hashes"
    assert lines[4] == footer
    sites = [gaps.family_site_row(1, "g1.fa", "chr2", 150_002, 151_343, 86, 24, 171, 75, 4, ["6"], "block"),
             gaps.family_site_row(2, "g1.fa", "chr1", 10, 50, 5, 24, 9, 3, 4, [], "gap")]
    text = gaps.family_sites_table(sites, 24, 16, 4, 1000, 3, 2, 34)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 5
    assert lines[0] == "\t".join(gaps.FAMILY_SITE_COLUMNS)
    assert lines[1] == "1\tg1.fa\tchr2\t150002\t151367\t1365\t86\t171\t75\t7.9\t6\tblock"
    assert lines[2] == "2\tg1.fa\tchr1\t10\t74\t64\t5\t.\t.\t.\t.\tgap"
    assert lines[3] == footer
    empty = "# k 150, rate 1, min_hits 1, step 0, arrays 0, families 0, set 0 hashes\n"
    assert gaps.families_table([], 150, 1, 1, 0, 0) == "\t".join(gaps.FAMILY_COLUMNS) + "\n" + empty
    assert gaps.family_sites_table([], 150, 1, 1, 0, 0, 0, 0) == "\t".join(gaps.FAMILY_SITE_COLUMNS) + "\n" + empty


def _fastas(tmp_path):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    return paths


def test_the_switch_implies_the_periods_and_is_listed(tmp_path, capsys):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    args = parser.parse_args(paths + ["-d", "1"])
    assert args.gap_families is False
    cli.check_reports(parser, args)
    assert not args.gap_families and not args.gap_periods and not args.gaps
    args = parser.parse_args(paths + ["-d", "1", "--gap-periods"])
    cli.check_reports(parser, args)
    assert args.gap_periods and not args.gap_families                                # the periods alone stay what they were
    args = parser.parse_args(paths + ["-d", "1", "--gap-families", "--gap-links-rate", "8", "--gap-links-min", "2", "--gap-sites-step", "500"])
    cli.check_reports(parser, args)
    assert args.gap_families and args.gap_periods and args.gaps and not args.gap_links and not args.gap_copies and not args.gap_copy_sites
    assert (args.gap_links_rate, args.gap_links_min, args.gap_sites_step) == (8, 2, 500)
    assert cli.main(paths + ["-d", "1", "--gap-families", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_periods -> gap_families")
    assert cli.main(paths + ["-d", "1", "--gap-copy-sites", "--gap-links", "--gap-families", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_copies -> gap_copy_sites -> gap_periods -> gap_families")
    assert cli.main(paths + ["-d", "1", "--gap-periods", "-n"]) == 0                 # without the switch: the list it had
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_periods")
    for bad in (["--gap-links-min", "0"], ["--gap-links-rate", "0"], ["--gap-sites-step", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(paths + ["-d", "1", "--gap-families", "-n"] + bad)


def test_the_switch_is_refused_without_a_filter_and_under_several_ranks(tmp_path, capsys, monkeypatch):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-families", "--no-common"]))
    assert "--gap-families reads the common Bloom filter: not with --no-common" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-families"]))
    err = capsys.readouterr().err
    assert "--gap-families works from the genomes resident on one GPU" in err
    assert "--families-out <prefix>.gap_families.tsv" in err and "--family-sites-out <prefix>.gap_family_sites.tsv" in err
    monkeypatch.setenv("WORLD_SIZE", "1")
    cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-families"]))             # one rank: accepted


def test_the_tool_takes_its_two_options_alone_and_together():
    base = ["--tsv", "g.synteny_blocks.tsv", "--fastas", "a.fa", "b.fa", "--common", "g.common.bf"]
    p = gaps.build_parser()
    args = p.parse_args(base)
    assert args.families_out is None and args.family_sites_out is None
    args = p.parse_args(base + ["--families-out", "f.tsv", "--sites-step", "500"])
    assert (args.families_out, args.family_sites_out, args.sites_step, args.periods_out) == ("f.tsv", None, 500, None)
    args = p.parse_args(base + ["--family-sites-out", "s.tsv"])
    assert (args.families_out, args.family_sites_out, args.links_rate, args.links_min, args.sites_step) == (None, "s.tsv", 16, 4, 1000)
    args = p.parse_args(base + ["--links-out", "l.tsv", "--periods-out", "p.tsv", "--families-out", "f.tsv", "--family-sites-out", "s.tsv"])
    assert (args.links_out, args.periods_out, args.families_out, args.family_sites_out) == ("l.tsv", "p.tsv", "f.tsv", "s.tsv")
    for option in ("--families-out", "--family-sites-out"):
        with pytest.raises(SystemExit):
            p.parse_args(base + [option])
        with pytest.raises(SystemExit):
            gaps.main(base + [option, "x.tsv", "--links-min", "0"])
        with pytest.raises(SystemExit):
            gaps.main(base + [option, "x.tsv", "--sites-step", "-1"])
        with pytest.raises(FileNotFoundError):                                      # parsed and accepted: main gets as far as its inputs
            gaps.main(["--tsv", "/nonexistent/t.tsv", "--fastas", "/nonexistent/a.fa", "--common", "/nonexistent/c.bf", option, "x.tsv"])


def test_families_refuses_bad_parameters_before_any_device_work():
    for kw in ({"rate": 0}, {"min_hits": 0}, {"step": -1}):
        with pytest.raises(ValueError, match="families"):
            gaps.families(None, {}, 24, [], [], [], **kw)
    with pytest.raises(ValueError, match="one period row per gap"):
        gaps.families(None, {}, 24, [ARRAY], [], [])
    from ntsynt_amd import pipeline
    with pytest.raises(ValueError, match="gap_families needs gap_periods"):
        pipeline.run(["a.fa", "b.fa"], gap_families=1000, backend=object())
    with pytest.raises(ValueError, match="gap_families = step"):
        pipeline.run(["a.fa", "b.fa"], gap_periods=(16, 4), gap_families=-1, backend=object())


def test_periods_hands_its_sampling_back_only_when_asked():
    sampling = ([], [])
    assert gaps.periods(None, {}, 24, [], sampling=sampling) == []                   # by default: what it returned
    assert gaps.periods(None, {}, 24, [], sampling=sampling, with_sampling=True) == ([], sampling)

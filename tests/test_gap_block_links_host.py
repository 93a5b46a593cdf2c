"""Gap block links, the host side (ntsynt_amd/gaps.py blocks_in_span / block_placement / gap_to_block / block_links_table, the command
line's switches): no GPU."""
import numpy as np
import pytest

from ntsynt_amd import cli, gaps
from ntsynt_amd.assess import BlockRow


def _block(block_id, genome, contig, start, end):
    return BlockRow(block_id, genome, contig, start, end, "+", "", "")


def test_blocks_in_span():
    table = [_block("7", "a.fa", "chr1", 1000, 2000),
             _block("7", "b.fa", "chr1", 1100, 2100),
             _block("3", "a.fa", "chr1", 2000, 3000),                           # touches block 7
             _block("9", "a.fa", "chr1", 2500, 4000),                           # overlaps block 3
             _block("1", "a.fa", "chr2", 0, 10_000),
             _block("4", "a.fa", "chr1", 5000, 6000)]
    span = lambda a, b, genome="a.fa", contig="chr1": gaps.blocks_in_span(table, genome, contig, a, b)   # noqa: E731
    assert span(1500, 1600) == ["7"]
    assert span(1999, 2000) == ["7"] and span(2000, 2001) == ["3"]             # half-open on both sides: a touching block is not in
    assert span(1999, 2001) == ["7", "3"]
    assert span(2400, 2600) == ["3", "9"] and span(0, 10**9) == ["7", "3", "9", "4"]      # file order, not coordinate order
    assert span(3000, 3001) == ["9"] and span(4000, 5000) == [] and span(0, 1000) == []
    assert span(1500, 1600, genome="b.fa") == ["7"] and span(1000, 1100, genome="b.fa") == []
    assert span(0, 10, contig="chr2") == ["1"] and span(0, 10, genome="c.fa") == []
    again = table + [_block("3", "a.fa", "chr1", 2900, 3100)]                   # an id twice on one contig: named once
    assert gaps.blocks_in_span(again, "a.fa", "chr1", 2000, 3100) == ["3", "9"]


def test_block_placement():
    gap = {"genome": "a.fa", "left_block": "3", "right_block": "4"}
    assert gaps.block_placement(gap, "a.fa", ["9"]) == "own"
    assert gaps.block_placement(gap, "a.fa", ["3"]) == "own"                   # the own genome comes first
    assert gaps.block_placement(gap, "a.fa", []) == "own"
    assert gaps.block_placement(gap, "b.fa", ["3"]) == "flank" and gaps.block_placement(gap, "b.fa", ["9", "4"]) == "flank"
    assert gaps.block_placement(gap, "b.fa", ["9"]) == "other" and gaps.block_placement(gap, "b.fa", []) == "other"
    edge = {"genome": "a.fa", "left_block": ".", "right_block": "4"}
    assert gaps.block_placement(edge, "b.fa", ["4"]) == "flank" and gaps.block_placement(edge, "b.fa", ["."]) == "other"
    unplaced = {"genome": "a.fa", "left_block": ".", "right_block": "."}
    assert gaps.block_placement(unplaced, "b.fa", ["."]) == "other" and gaps.block_placement(unplaced, "b.fa", ["1"]) == "other"
    assert gaps.block_placement(unplaced, "a.fa", ["1"]) == "own"


def _row(**over):
    row = {"genome": "b.fa", "contig": "chr1", "start": 90_000, "end": 96_000, "left_block": "0", "right_block": "1", "target_genome": "a.fa",
           "target_contig": "chr2", "target_start": 12, "target_end": 299_990, "blocks": "2", "anchors": 243, "orientation": "+", "from": 90_012,
           "to": 95_981, "from_t": 100_012, "to_t": 105_981, "sampled": 246, "target_hits": 251, "placement": "other"}
    row.update(over)
    return row


def test_block_links_table_formatting():
    text = gaps.block_links_table([_row(), _row(target_genome="b.fa", anchors=246, placement="own", blocks="2,5")], 24, 16, 4, 4194304, 1234)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 5
    assert lines[0].split("\t") == list(gaps.BLOCK_LINK_COLUMNS)
    assert gaps.BLOCK_LINK_COLUMNS == ("genome", "contig", "start", "end", "left_block", "right_block", "target_genome", "target_contig", "target_start",
                                       "target_end", "blocks", "anchors", "orientation", "from", "to", "from_t", "to_t", "sampled", "target_hits",
                                       "placement")
    assert lines[1] == "b.fa\tchr1\t90000\t96000\t0\t1\ta.fa\tchr2\t12\t299990\t2\t243\t+\t90012\t95981\t100012\t105981\t246\t251\tother"
    assert lines[2] == "b.fa\tchr1\t90000\t96000\t0\t1\tb.fa\tchr2\t12\t299990\t2,5\t246\t+\t90012\t95981\t100012\t105981\t246\t251\town"
    assert lines[3] == "# k 24, rate 16, min_anchors 4, filter 4194304 bits, set 1234 hashes"
    assert gaps.block_links_table([], 150, 1, 1, 64, 0) == "\t".join(gaps.BLOCK_LINK_COLUMNS) + "\n# k 150, rate 1, min_anchors 1, filter 64 bits, set 0 hashes\n"


def test_only_gap_to_block_links_are_kept():
    from ntsynt_amd.device import LINK_DTYPE
    n = 3                                                                       # lists 0..2: the genomes' gaps; 3..5: their block intervals
    pairs = [(0, 5, 1, 2), (0, 5, 3, 0), (0, 5, 4, 1), (0, 6, 5, 0), (1, 0, 2, 0), (1, 0, 4, 7), (2, 9, 3, 1), (2, 9, 5, 2), (3, 0, 4, 0), (3, 1, 5, 2),
             (4, 0, 5, 0)]
    found = np.zeros(len(pairs), dtype=LINK_DTYPE)
    for i, (la, iva, lb, ivb) in enumerate(pairs):
        found[i]["list_a"], found[i]["iv_a"], found[i]["list_b"], found[i]["iv_b"], found[i]["anchors"] = la, iva, lb, ivb, 10 + i
    kept = gaps.gap_to_block(found, n)
    assert kept.dtype == LINK_DTYPE
    assert [tuple(int(r[f]) for f in ("list_a", "iv_a", "list_b", "iv_b")) for r in kept] == \
        [(0, 5, 3, 0), (0, 5, 4, 1), (0, 6, 5, 0), (1, 0, 4, 7), (2, 9, 3, 1), (2, 9, 5, 2)]      # the gap's own genome (0 -> 3, 2 -> 5) stays
    assert [int(r["anchors"]) for r in kept] == [11, 12, 13, 15, 16, 17]       # whole rows, in the join's order
    assert gaps.gap_to_block(found[:0], n).size == 0
    assert gaps.gap_to_block(found, 6).size == 0                                # every list a gap list: nothing points into a block
    assert gaps.MAX_BLOCK_LINK_GENOMES == 32


def _fastas(tmp_path):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    return paths


def test_the_switch_implies_gap_links_and_shares_its_settings(tmp_path, capsys):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    args = parser.parse_args(paths + ["-d", "1"])
    assert args.gap_block_links is False
    cli.check_reports(parser, args)
    assert not args.gap_block_links and not args.gap_links and not args.gaps
    args = parser.parse_args(paths + ["-d", "1", "--gap-block-links", "--gap-links-rate", "8", "--gap-links-min", "2"])
    assert args.gap_block_links and not args.gap_links                          # (what it implies is settled by check_reports)
    cli.check_reports(parser, args)
    assert args.gap_block_links and args.gap_links and args.gaps and (args.gap_links_rate, args.gap_links_min) == (8, 2)
    args = parser.parse_args(paths + ["-d", "1", "--gap-links"])
    cli.check_reports(parser, args)
    assert args.gap_links and not args.gap_block_links                          # not the other way round
    # the dry run's list: the switch alone brings gaps and gap_links, and comes last
    assert cli.main(paths + ["-d", "1", "--gap-block-links", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links -> gap_block_links")
    assert cli.main(paths + ["-d", "1", "--gap-links", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links")
    for bad in (["--gap-links-rate", "0"], ["--gap-links-min", "0"]):
        with pytest.raises(SystemExit):
            cli.main(paths + ["-d", "1", "--gap-block-links", "-n"] + bad)


def test_the_switch_is_refused_without_a_filter_and_under_several_ranks(tmp_path, capsys, monkeypatch):
    paths = _fastas(tmp_path)
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-block-links", "--no-common"]))
    assert "--gap-block-links reads the common Bloom filter: not with --no-common" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-block-links"]))
    err = capsys.readouterr().err
    assert "--gap-block-links works from the genomes resident on one GPU" in err and "--block-links-out" in err
    monkeypatch.setenv("WORLD_SIZE", "1")
    cli.check_reports(parser, parser.parse_args(paths + ["-d", "1", "--gap-block-links"]))      # one rank: accepted

"""Gap links, the host side (ntsynt_amd/gaps.py links_table / placement / orientation, the command line's switches): no GPU."""
import pytest

from ntsynt_amd import cli, gaps


def _gap(left, right):
    return {"left_block": left, "right_block": right}


def _row(**over):
    row = dict(genome_a="a.fa", contig_a="chr1", start_a=100, end_a=6100, left_a="3", right_a="4", genome_b="b.fa", contig_b="chr2", start_b=7,
               end_b=6007, left_b="4", right_b="3", anchors=212, orientation="-", from_a=130, to_a=6090, from_b=20, to_b=5999, sampled_a=260,
               sampled_b=255, placement="same")
    row.update(over)
    return row


def test_links_table_formatting():
    text = gaps.links_table([_row(), _row(genome_b="c.fa", anchors=4, orientation=".", placement="other", left_b=".", right_b=".")], 24, 16, 4, 4194304)
    lines = text.split("\n")
    assert text.endswith("\n") and lines[-1] == "" and len(lines) == 5
    assert lines[0].split("\t") == list(gaps.LINK_COLUMNS)
    assert gaps.LINK_COLUMNS == ("genome_a", "contig_a", "start_a", "end_a", "left_a", "right_a", "genome_b", "contig_b", "start_b", "end_b", "left_b",
                                 "right_b", "anchors", "orientation", "from_a", "to_a", "from_b", "to_b", "sampled_a", "sampled_b", "placement")
    assert lines[1] == "a.fa\tchr1\t100\t6100\t3\t4\tb.fa\tchr2\t7\t6007\t4\t3\t212\t-\t130\t6090\t20\t5999\t260\t255\tsame"
    assert lines[2] == "a.fa\tchr1\t100\t6100\t3\t4\tc.fa\tchr2\t7\t6007\t.\t.\t4\t.\t130\t6090\t20\t5999\t260\t255\tother"
    assert lines[3] == "# k 24, rate 16, min_anchors 4, filter 4194304 bits"
    assert gaps.links_table([], 150, 1, 1, 64) == "\t".join(gaps.LINK_COLUMNS) + "\n# k 150, rate 1, min_anchors 1, filter 64 bits\n"


def test_placement():
    assert gaps.placement(_gap("3", "4"), _gap("3", "4")) == "same"
    assert gaps.placement(_gap("3", "4"), _gap("4", "3")) == "same"                 # the other genome runs the other way
    assert gaps.placement(_gap("3", "4"), _gap("3", "5")) == "other"
    assert gaps.placement(_gap("3", "4"), _gap("4", "5")) == "other"
    assert gaps.placement(_gap(".", "4"), _gap("4", ".")) == "same"                 # a record's end on both sides
    assert gaps.placement(_gap(".", "4"), _gap("4", "4")) == "other"
    assert gaps.placement(_gap(".", "."), _gap(".", ".")) == "other"                # unplaced records: no flank to share
    assert gaps.placement(_gap(".", "."), _gap(".", "4")) == "other"


def test_orientation():
    assert gaps.orientation(5, 1) == "+"
    assert gaps.orientation(1, 5) == "-"
    assert gaps.orientation(3, 3) == "."
    assert gaps.orientation(0, 0) == "."                                            # one anchor, or all offsets equal
    assert gaps.orientation(1, 0) == "+" and gaps.orientation(0, 1) == "-"


def test_defaults_and_the_switch_implies_gaps(tmp_path, capsys):
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    args = cli.build_parser().parse_args(paths + ["-d", "1"])
    assert (args.gap_links, args.gap_links_rate, args.gap_links_min) == (False, 16, 4) and not args.gaps
    assert (gaps.LINKS_RATE, gaps.LINKS_MIN) == (16, 4)
    args = cli.build_parser().parse_args(paths + ["-d", "1", "--gap-links", "--gap-links-rate", "8", "--gap-links-min", "2"])
    assert (args.gap_links, args.gap_links_rate, args.gap_links_min) == (True, 8, 2)
    # the dry run's list: --gap-links alone brings the gaps stage, and comes last
    assert cli.main(paths + ["-d", "1", "--gap-links", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps -> gap_links")
    assert cli.main(paths + ["-d", "1", "--assess", "--gaps", "--gap-links", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> assess -> gaps -> gap_links")
    assert cli.main(paths + ["-d", "1", "--gaps", "-n"]) == 0
    assert capsys.readouterr().out.strip().endswith("ntsynt_synteny -> gaps")
    for bad in (["--gap-links-rate", "0"], ["--gap-links-min", "0"]):
        with pytest.raises(SystemExit):
            cli.main(paths + ["-d", "1", "--gap-links", "-n"] + bad)
    with pytest.raises(SystemExit):
        cli.main(paths + ["-d", "1", "--gap-links", "--no-common", "-n"])
    assert "--gap-links reads the common Bloom filter" in capsys.readouterr().err

"""The host side of the block identity (ntsynt_amd/assess.py identity_row / identity_table, the switches of ntSynt and
ntsynt_block_stats): the file's arithmetic by hand, and argument parsing -- ranges, refusal under several ranks, --dry-run.  No GPU."""
import pytest

from ntsynt_amd import assess, cli
from tests import identity_brute as B


def row(**kw):
    r = dict(block_id="7", genome_a="a.fa", genome_b="b.fa", orientation="+", length_a=10_000, length_b=10_050, anchors=30, segments=29, aligned=25,
             aligned_a=8_000, aligned_b=8_010, edits=81, backward=1, long=1, offband=1, invalid=0, overband=1)
    r.update(kw)
    return r


def test_columns_are_the_issue_s():
    assert assess.IDENTITY_COLUMNS == B.COLUMNS
    assert "\t".join(assess.IDENTITY_COLUMNS) == ("block_id\tgenome_a\tgenome_b\torientation\tlength_a\tlength_b\tanchors\tsegments\taligned\taligned_a\t"
                                                  "aligned_b\tedits\tidentity\tcovered_a\tcovered_b\tbackward\tlong\toffband\tinvalid\toverband")


def test_identity_row_by_hand():
    # M = 8010; (10^6 * 7929) // 8010 = 989887; covered: 8000 / 10000 = 80.0 %, (1000 * 8010) // 10050 = 797 -> 79.7 %
    assert assess.identity_row(row()) == "7\ta.fa\tb.fa\t+\t10000\t10050\t30\t29\t25\t8000\t8010\t81\t0.989887\t80.0\t79.7\t1\t1\t1\t0\t1"
    assert assess.identity_row(row()) == B.format_row(row())


def test_no_edit_and_nothing_aligned():
    f = assess.identity_row(row(edits=0)).split("\t")
    assert f[12] == "1.000000"
    f = assess.identity_row(row(aligned=0, aligned_a=0, aligned_b=0, edits=0)).split("\t")
    assert f[12] == "." and f[13] == "0.0" and f[14] == "0.0"
    f = assess.identity_row(row(edits=8010)).split("\t")
    assert f[12] == "0.000000"
    f = assess.identity_row(row(aligned_a=1, aligned_b=1, edits=1, length_a=0)).split("\t")
    assert f[13] == "."                                      # an interval clipped to nothing


@pytest.mark.parametrize("aligned, length, shown", [(999, 1000, "99.9"), (9999, 10000, "99.9"), (1, 1001, "0.0"), (1, 1000, "0.1"), (1000, 1000, "100.0"),
                                                    (2, 3, "66.6"), (5, 1000, "0.5")])
def test_covered_rounds_down(aligned, length, shown):
    f = assess.identity_row(row(aligned_a=aligned, length_a=length)).split("\t")
    assert f[13] == shown


def test_table_and_footer():
    text = assess.identity_table([row(), row(block_id="8", orientation="-")], 21, 16, 31, 4096)
    lines = text.split("\n")
    assert lines[0] == "\t".join(assess.IDENTITY_COLUMNS) and len(lines) == 5 and lines[4] == ""
    assert lines[3] == "# k 21, rate 16, band 31, max_len 4096"
    assert lines[2].split("\t")[:4] == ["8", "a.fa", "b.fa", "-"]
    assert assess.identity_table([], 19, 4, 7, 100) == "\t".join(assess.IDENTITY_COLUMNS) + "\n# k 19, rate 4, band 7, max_len 100\n"


def parse(argv, monkeypatch, world=None):
    if world:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    else:
        monkeypatch.delenv("WORLD_SIZE", raising=False)
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_reports(parser, args)
    return args


def test_switch_defaults_and_ranges(monkeypatch, capsys):
    args = parse(["a.fa", "b.fa", "-d", "1", "--block-identity"], monkeypatch)
    assert (args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len) == (21, 16, 31, 4096) and not args.assess
    assert not parse(["a.fa", "b.fa", "-d", "1"], monkeypatch).block_identity
    parse(["a.fa", "b.fa", "-d", "1", "--block-identity", "--identity-band", "1", "--identity-max-len", "65535", "--identity-rate", "1"], monkeypatch)
    for bad in (["--identity-band", "0"], ["--identity-band", "32"], ["--identity-max-len", "0"], ["--identity-max-len", "65536"],
                ["--identity-rate", "0"], ["--identity-k", "0"]):
        with pytest.raises(SystemExit) as err:
            parse(["a.fa", "b.fa", "-d", "1", "--block-identity"] + bad, monkeypatch)
        assert err.value.code == 2
        assert bad[0] in capsys.readouterr().err
    parse(["a.fa", "b.fa", "-d", "1", "--identity-band", "99"], monkeypatch)      # without the switch the values are not looked at


def test_refused_under_several_ranks(monkeypatch, capsys):
    with pytest.raises(SystemExit) as err:
        parse(["a.fa", "b.fa", "-d", "1", "--block-identity"], monkeypatch, world=2)
    assert err.value.code == 2 and "--block-identity works from the genomes resident on one GPU" in capsys.readouterr().err


def test_dry_run_lists_the_stage(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--assess", "--block-identity", "--gaps"]) == 0
    out = capsys.readouterr().out
    assert "ntsynt_synteny -> assess -> block_identity -> gaps" in out
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run"]) == 0
    assert "block_identity" not in capsys.readouterr().out


def test_tool_refuses_bad_parameters(capsys):
    for argv in (["--tsv", "x.tsv", "--fai", "a.fai", "--identity-out", "o.tsv"],
                 ["--tsv", "x.tsv", "--fai", "a.fai", "--fastas", "a.fa", "--identity-out", "o.tsv", "--identity-band", "40"]):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
    assert "--identity" in capsys.readouterr().err


def test_brute_force_edit_distance_by_hand():
    import numpy as np
    s = lambda t: np.frombuffer(t.encode(), dtype=np.uint8)   # noqa: E731
    assert B.levenshtein(s("ACGT"), s("ACGT")) == 0
    assert B.levenshtein(s("ACGT"), s("AGT")) == 1
    assert B.levenshtein(s("A"), s("CCCCA")) == 4
    assert B.levenshtein(s("AAAA"), s("TTTT")) == 4
    assert B.levenshtein(s("ACGTACGT"), s("CGTACGTA")) == 2
    assert B.revcomp(s("AACGN")).tobytes() == b"NCGTT"
    segs, per = B.brute_segments([(1, 0, 0), (2, 0, 10), (3, 0, 30)], [(1, 0, 79), (2, 0, 69), (3, 0, 48)], [0], [100], [1], 21, 31, 4096)
    assert per == [3] and segs == [(0, 0, 10, 0, 10, B.CANDIDATE), (0, 10, 20, 10, 21, B.CANDIDATE)]

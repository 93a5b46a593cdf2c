"""The host side of the block wide variants (docs/design/04_19_block_wide_variants.md): argument parsing -- refused without
--identity-max-edits, refused under several ranks, --block-variants with E still refused --, the tool's and pipeline.run's refusals,
the --dry-run stage text with and without the switch, the footer of wide_variants_table, block_wide_variants(max_edits=0).  These
need the feature.  The last test checks the reference alone: the script set and the ops of tests/wide_variants_brute.py against a case
worked out by hand, as tests/test_block_identity_wide_host.py checks tests/wide_brute.py -- it runs nothing of ntsynt_amd.  No GPU."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from tests import identity_brute as B
from tests import wide_variants_brute as WV

STAGE = "block_wide_variants (edit_script_plan, edit_script, edit_wide_script_plan, edit_wide_script)"


def parse(argv, monkeypatch, world=None):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if world:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_reports(parser, args)
    return args


def test_switch_needs_e(monkeypatch, capsys):
    base = ["a.fa", "b.fa", "-d", "1", "--block-wide-variants"]
    args = parse(base + ["--identity-max-edits", "1023"], monkeypatch)
    assert args.block_wide_variants and args.identity_max_edits == 1023 and not args.block_identity and not args.block_variants
    assert parse(base + ["--identity-max-edits", "63", "--block-identity"], monkeypatch).block_identity
    assert not parse(["a.fa", "b.fa", "-d", "1"], monkeypatch).block_wide_variants
    for extra in ([], ["--block-identity"], ["--identity-max-edits", "0"]):
        with pytest.raises(SystemExit) as err:
            parse(base + extra, monkeypatch)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert "--identity-max-edits" in said and "--block-variants" in said, said
    for bad in (["--identity-max-edits", "62"], ["--identity-max-edits", "1024"], ["--identity-band", "7", "--identity-max-edits", "14"]):
        with pytest.raises(SystemExit) as err:
            parse(base + bad, monkeypatch)
        assert err.value.code == 2 and "--identity-max-edits" in capsys.readouterr().err


def test_refused_under_several_ranks(monkeypatch, capsys):
    with pytest.raises(SystemExit) as err:
        parse(["a.fa", "b.fa", "-d", "1", "--block-wide-variants", "--identity-max-edits", "1023"], monkeypatch, world=2)
    assert err.value.code == 2
    said = capsys.readouterr().err
    assert "--block-wide-variants" in said and "one rank" in said and "--wide-variants-out" in said


def test_block_variants_with_e_is_still_refused(monkeypatch, capsys):
    for switches in (["--block-variants"], ["--block-variants", "--block-wide-variants"], ["--block-identity", "--block-variants", "--block-wide-variants"]):
        with pytest.raises(SystemExit) as err:
            parse(["a.fa", "b.fa", "-d", "1", "--identity-max-edits", "1023"] + switches, monkeypatch)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert "not listed yet" in said and "--block-wide-variants" in said
    assert "not listed yet" in assess.WIDE_NOT_WITH_VARIANTS


def test_tool_refusals(capsys):
    base = ["--tsv", "x.tsv", "--fai", "a.fai"]
    for argv, words in ((base + ["--fastas", "a.fa", "--wide-variants-out", "w.tsv"], ("--identity-max-edits", "--variants-out")),
                        (base + ["--fastas", "a.fa", "--wide-variants-out", "w.tsv", "--identity-max-edits", "62"], ("--identity-max-edits",)),
                        (base + ["--wide-variants-out", "w.tsv", "--identity-max-edits", "1023"], ("--fastas",)),
                        (base + ["--fastas", "a.fa", "--wide-variants-out", "w.tsv", "--variants-out", "v.tsv", "--identity-max-edits", "100"],
                         ("not listed yet",))):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert all(w in said for w in words), (argv, said)


def test_pipeline_refusals():
    from ntsynt_amd import pipeline

    for kwargs, word in ((dict(block_wide_variants=(21, 16, 31, 4096, 0)), "--identity-max-edits"),
                         (dict(block_wide_variants=(21, 16, 31, 4096)), "max_edits"),
                         (dict(block_wide_variants=(21, 16, 31, 4096, 62)), "--identity-max-edits"),
                         (dict(block_wide_variants=(21, 16, 31, 4096, 1023), block_variants=(21, 16, 31, 4096)), "not listed yet"),
                         (dict(block_wide_variants=(21, 16, 31, 4096, 1023), block_identity=(21, 16, 31, 4096)), "the same"),
                         (dict(block_wide_variants=(21, 16, 31, 4096, 1023), block_identity=(21, 16, 31, 4096, 63)), "the same"),
                         (dict(block_identity=(21, 16, 31, 4096, 1023), block_variants=(21, 16, 31, 4096)), "not listed yet")):
        with pytest.raises(ValueError) as err:
            pipeline.run(["a.fa", "b.fa"], k=24, w=100, prefix="x", backend=object(), **kwargs)    # (refused before the backend is used)
        assert word in str(err.value), err.value


def test_dry_run_lists_the_stage_only_with_the_switch(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    common = paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--gaps"]
    assert cli.main(common + ["--block-wide-variants", "--identity-max-edits", "1023"]) == 0
    assert f"ntsynt_synteny -> {STAGE} -> gaps" in capsys.readouterr().out
    assert cli.main(common + ["--block-identity", "--block-wide-variants", "--identity-max-edits", "1023"]) == 0
    assert f"block_identity -> block_identity_wide (edit_wide_plan, edit_wide) -> {STAGE} -> gaps" in capsys.readouterr().out
    assert cli.main(common + ["--block-identity", "--identity-max-edits", "1023"]) == 0
    out = capsys.readouterr().out
    assert "block_identity_wide (edit_wide_plan, edit_wide) -> gaps" in out and "block_wide_variants" not in out and "edit_wide_script" not in out
    assert cli.main(common + ["--block-variants"]) == 0
    out = capsys.readouterr().out
    assert "block_variants -> gaps" in out and "block_wide_variants" not in out


def test_table_footer_and_columns():
    row = dict(block_id="3", genome_a="a.fa", contig_a="chr1", pos_a=100, genome_b="b.fa", contig_b="chr2", pos_b=140, orientation="-", type="ins",
               length=40, seq_a="-", seq_b="ACGT" * 10)
    text = assess.wide_variants_table([row], 21, 16, 31, 4096, 1023)
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.VARIANT_COLUMNS) and len(assess.VARIANT_COLUMNS) == 12
    assert lines[1] == assess.variant_row(row) and lines[-1] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023" and text.endswith("\n")
    assert lines[:-1] == assess.variants_table([row], 21, 16, 31, 4096).splitlines()[:-1]
    assert assess.wide_variants_table([], 21, 16, 7, 100, 15).splitlines() == ["\t".join(assess.VARIANT_COLUMNS), "# k 21, rate 16, band 7, max_len 100, max_edits 15"]


def test_block_wide_variants_needs_e():
    with pytest.raises(ValueError) as err:
        assess.block_wide_variants(None, {}, [], 21, 16, 31, 4096, max_edits=0)
    assert "block_variants" in str(err.value)
    with pytest.raises(ValueError) as err:
        assess.block_wide_variants(None, {}, [], 21, 16, 31, 4096)
    assert "block_variants" in str(err.value)
    with pytest.raises(ValueError) as err:
        assess.block_wide_variants(None, {}, [], 21, 16, 31, 4096, max_edits=62)
    assert "--identity-max-edits" in str(err.value)


def test_script_set_by_hand():
    """the reference only (tests/wide_variants_brute.py; nothing of the feature runs here).  Band 1 (2 W + 1 = 3): offband with a
    distance; a candidate with D + |delta| = 3 is nts_edit_script's, with 5 it is a member"""
    s = lambda text: np.frombuffer(text.encode(), dtype=np.uint8)                              # noqa: E731
    a = s("AAAA" "CCCC" "GGGG" "TTTT" "ACGT")
    b = s("AAAA" "CCTTCC" "GCCG" "TGGCA" "ACGT")
    segs = [(0, 0, 4, 0, 4, B.CANDIDATE),                     # equal: D = 0
            (0, 4, 4, 4, 6, B.OFFBAND),                       # D = 2: offband, a member
            (0, 8, 4, 10, 4, B.CANDIDATE),                    # D = 2, delta 0: 2 <= 3, nts_edit_script's
            (0, 12, 4, 14, 5, B.CANDIDATE),                   # TTTT / TGGCA: D = 4, delta 1: 5 > 3, a member
            (0, 16, 4, 19, 4, B.BACKWARD)]
    final = [0, 2, 2, 4, B.PASSED]
    assert [WV.in_script_set(seg, d, 1) for seg, d in zip(segs, final)] == [False, True, False, True, False]
    assert not WV.in_script_set(segs[1], B.OVERBAND, 1) and not WV.in_script_set(segs[1], B.INVALID, 1) and not WV.in_script_set(segs[1], B.PASSED, 1)
    ops, first, members = WV.expected_ops(a, b, [(0, a.size)], [(0, b.size)], [0], segs, final, 1)
    assert members == [1, 3] and first == [0, 0, 2, 2, 6, 6]
    assert ops[:2] == [(1, 2, 2, 3, 0xFF, 3), (1, 2, 3, 3, 0xFF, 3)]                          # CCCC / CCTTCC: two T inserted in front of A[2]
    assert [op[0] for op in ops[2:]] == [3] * 4

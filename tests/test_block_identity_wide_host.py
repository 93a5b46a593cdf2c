"""The host side of the wide pass of the block identity (docs/design/04_18_block_identity_wide.md): tests/wide_brute.py against cases
computed by hand -- the precedence of the kinds with E > 0, the work set, the sums --, the range of --identity-max-edits, the footer with
and without E, and argument parsing: refusals of E out of range and of E together with the block variants, --dry-run.  No GPU."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from tests import identity_brute as B
from tests import wide_brute as W


def s(text):
    return np.frombuffer(text.encode(), dtype=np.uint8)


def test_wide_result_by_hand():
    assert W.wide_result(s("ACGT"), s("ACGT"), 3) == 0
    assert W.wide_result(s("ACGT"), s("AGGT"), 3) == 1
    assert W.wide_result(s("A"), s("ACGT"), 3) == 3                         # three insertions: D = E
    assert W.wide_result(s("A"), s("ACGTA"), 3) == B.OVERBAND               # four: D = E + 1
    assert W.wide_result(s("AAAA"), s("CCCC"), 3) == B.OVERBAND
    assert W.wide_result(s("ANGT"), s("ACGT"), 3) == B.INVALID
    assert W.wide_result(s("AAAA"), s("CCCN"), 3) == B.INVALID              # invalid before overband
    assert W.wide_result(s("ACGTACGT"), s("ACGT"), 4) == 4                  # a pure deletion of four bases


def test_kinds_work_set_and_sums_by_hand():
    "band 1, E = 3: one interval of A = AAAACCCCGGGGTTTTACGT against a B built segment by segment"
    a = s("AAAA" "CCCC" "G" "TTTT" "ACGT" "AC" "GGGG")
    b = s("AAAA" "CCTTCC" "GACGTA" "TTTN" "TGCA" "ACGTAC" "GCCG")
    #      equal  +2       +5       N      4 subs  +4      2 subs
    segs = [(0, 0, 4, 0, 4, B.CANDIDATE),                     # equal: the narrow pass aligns it, D = 0
            (0, 4, 4, 4, 6, B.OFFBAND),                       # |delta| = 2 > band, <= E: work set, D = 2
            (0, 8, 1, 10, 6, B.OFFBAND),                      # |delta| = 5 > E: stays passed, counted offband
            (0, 9, 4, 16, 4, B.CANDIDATE),                    # an invalid base: invalid in both passes
            (0, 13, 4, 20, 4, B.CANDIDATE),                   # D = 4 > E: overband in both passes
            (0, 17, 2, 24, 6, B.OFFBAND),                     # |delta| = 4 > E: passed
            (0, 19, 4, 30, 4, B.CANDIDATE),                   # D = 2: (2 + 0) // 2 = 1 <= band: the narrow pass aligns it
            (0, 0, 4, 0, -1, B.BACKWARD), (0, 0, 4, 0, 4, B.LONG), (0, 0, 4, 0, 4, 7)]
    narrow, final, per_iv, work = W.brute_wide(a, b, [(0, a.size)], [(0, b.size)], [0], segs, 1, 3)
    assert narrow == [0, B.PASSED, B.PASSED, B.INVALID, B.OVERBAND, B.PASSED, 2, B.PASSED, B.PASSED, B.NOT_CANDIDATE]
    assert final == [0, 2, B.PASSED, B.INVALID, B.OVERBAND, B.PASSED, 2, B.PASSED, B.PASSED, B.NOT_CANDIDATE]
    assert work == [1, 4]
    assert per_iv == [dict(aligned_a=12, aligned_b=14, edits=4, segments=10, aligned=3, backward=1, too_long=1, offband=2, invalid=1, overband=1)]
    # the narrow results are identity_brute's own
    assert B.brute_edit(a, b, [(0, a.size)], [(0, b.size)], [0], segs, 1)[0] == narrow


def test_offband_goes_before_invalid_and_invalid_before_overband():
    a, b = s("N"), s("NCCCCC")
    narrow, final, per_iv, work = W.brute_wide(a, b, [(0, 1)], [(0, 6)], [0], [(0, 0, 1, 0, 6, B.OFFBAND)], 1, 3)
    assert final == [B.PASSED] and per_iv[0]["offband"] == 1 and per_iv[0]["invalid"] == 0 and work == []
    narrow, final, per_iv, work = W.brute_wide(a, b, [(0, 1)], [(0, 6)], [0], [(0, 0, 1, 0, 4, B.OFFBAND)], 1, 3)
    assert final == [B.INVALID] and per_iv[0]["offband"] == 0 and per_iv[0]["invalid"] == 1 and work == [0]
    a, b = s("AAAAAAAN"), s("CCCCCCCC")
    _, final, per_iv, _ = W.brute_wide(a, b, [(0, 8)], [(0, 8)], [0], [(0, 0, 8, 0, 8, B.CANDIDATE)], 1, 3)
    assert final == [B.INVALID] and per_iv[0]["overband"] == 0


def test_flipped_segment_by_hand():
    a = s("ACGTTT")
    b = B.revcomp(s("ACGGGGTTT"))                             # the oriented B has three bases more
    narrow, final, _, work = W.brute_wide(a, b, [(0, 6)], [(0, 9)], [1], [(0, 0, 6, 0, 9, B.OFFBAND)], 1, 3)
    assert narrow == [B.PASSED] and final == [3] and work == [0]


def test_parameter_ranges():
    ok = assess.check_identity_parameters
    assert ok(21, 16, 31, 4096) is None and ok(21, 16, 31, 4096, 0) is None
    assert ok(21, 16, 31, 4096, 63) is None and ok(21, 16, 31, 4096, 1023) is None and ok(21, 16, 1, 4096, 3) is None
    for band, e in ((31, 62), (31, 1024), (31, 1), (31, -1), (1, 2), (7, 14)):
        assert "--identity-max-edits" in ok(21, 16, band, 4096, e), (band, e)
    assert "--identity-band" in ok(21, 16, 32, 4096, 1023)    # the first that is out of range
    with pytest.raises(ValueError):
        assess.block_identity(None, {}, [], 21, 16, 31, 4096, max_edits=62)


def test_footer_with_and_without_e():
    row = dict(block_id="3", genome_a="a.fa", genome_b="b.fa", orientation="+", length_a=1000, length_b=1040, anchors=5, segments=4, aligned=4,
               aligned_a=900, aligned_b=940, edits=49, backward=0, long=0, offband=0, invalid=0, overband=0)
    plain = assess.identity_table([row], 21, 16, 31, 4096)
    assert plain == assess.identity_table([row], 21, 16, 31, 4096, 0) == assess.identity_table([row], 21, 16, 31, 4096, max_edits=0)
    assert plain.splitlines()[-1] == "# k 21, rate 16, band 31, max_len 4096"
    wide = assess.identity_table([row], 21, 16, 31, 4096, 1023)
    assert wide.splitlines()[-1] == "# k 21, rate 16, band 31, max_len 4096, max_edits 1023"
    assert wide.splitlines()[:-1] == plain.splitlines()[:-1] and wide.splitlines()[1] == B.format_row(row)


# ---- argument parsing

def parse(argv, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_reports(parser, args)
    return args


def test_switch_default_and_ranges(monkeypatch, capsys):
    assert parse(["a.fa", "b.fa", "-d", "1", "--block-identity"], monkeypatch).identity_max_edits == 0
    assert parse(["a.fa", "b.fa", "-d", "1", "--block-identity", "--identity-max-edits", "63"], monkeypatch).identity_max_edits == 63
    assert parse(["a.fa", "b.fa", "-d", "1", "--block-identity", "--identity-max-edits", "1023"], monkeypatch).identity_max_edits == 1023
    parse(["a.fa", "b.fa", "-d", "1", "--block-identity", "--identity-band", "7", "--identity-max-edits", "15"], monkeypatch)
    for bad in (["--identity-max-edits", "62"], ["--identity-max-edits", "1024"], ["--identity-max-edits", "-5"],
                ["--identity-band", "7", "--identity-max-edits", "14"]):
        with pytest.raises(SystemExit) as err:
            parse(["a.fa", "b.fa", "-d", "1", "--block-identity"] + bad, monkeypatch)
        assert err.value.code == 2
        assert "--identity-max-edits" in capsys.readouterr().err


def test_refused_with_the_block_variants(monkeypatch, capsys):
    for switches in (["--block-identity", "--block-variants"], ["--block-variants"]):
        with pytest.raises(SystemExit) as err:
            parse(["a.fa", "b.fa", "-d", "1", "--identity-max-edits", "1023"] + switches, monkeypatch)
        assert err.value.code == 2
        assert "not listed yet" in capsys.readouterr().err
    parse(["a.fa", "b.fa", "-d", "1", "--block-identity", "--block-variants"], monkeypatch)    # without E the two still go together


def test_tool_refusals(capsys):
    base = ["--tsv", "x.tsv", "--fai", "a.fai", "--fastas", "a.fa"]
    for argv, word in ((base + ["--identity-out", "o.tsv", "--identity-max-edits", "62"], "--identity-max-edits"),
                       (base + ["--identity-out", "o.tsv", "--identity-max-edits", "1024"], "--identity-max-edits"),
                       (base + ["--identity-out", "o.tsv", "--variants-out", "v.tsv", "--identity-max-edits", "100"], "not listed yet"),
                       (base + ["--variants-out", "v.tsv", "--identity-max-edits", "100"], "not listed yet")):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
        assert word in capsys.readouterr().err


def test_pipeline_refusals():
    from ntsynt_amd import pipeline

    for kwargs, word in ((dict(block_identity=(21, 16, 31, 4096, 62)), "--identity-max-edits"),
                         (dict(block_identity=(21, 16, 31, 4096, 1023), block_variants=(21, 16, 31, 4096)), "not listed yet"),
                         (dict(block_identity=(21, 16, 31)), "max_edits")):
        with pytest.raises(ValueError) as err:
            pipeline.run(["a.fa", "b.fa"], k=24, w=100, prefix="x", backend=object(), **kwargs)    # (refused before the backend is used)
        assert word in str(err.value), err.value


def test_dry_run_shows_the_wide_pass_only_with_e(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--block-identity", "--identity-max-edits", "1023", "--gaps"]) == 0
    assert "block_identity -> block_identity_wide (edit_wide_plan, edit_wide) -> gaps" in capsys.readouterr().out
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--block-identity", "--gaps"]) == 0
    out = capsys.readouterr().out
    assert "block_identity -> gaps" in out and "block_identity_wide" not in out and "edit_wide" not in out

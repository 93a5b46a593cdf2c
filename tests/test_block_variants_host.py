"""The host side of the block variants (docs/design/04_17_block_variants.md): the brute force of tests/variants_brute.py checked
against itself and by hand -- applying a script to A gives B, its length is the edit distance, the canonical choices --, then
ntsynt_amd/assess.py variant_events / variant_row / variants_table on hand-made ops -- merging, both orientations' coordinates, the
first and last base of an interval, the empty table --, and argument parsing: ranges, --dry-run, refusal under several ranks.  No GPU."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from tests import identity_brute as B
from tests import variants_brute as V

OP = np.dtype([("seg", "<u4"), ("p", "<u4"), ("q", "<u4"), ("op", "u1"), ("base_a", "u1"), ("base_b", "u1"), ("pad", "u1")])
SEG = np.dtype([("iv_a", "<u4"), ("x", "<u4"), ("dx", "<u4"), ("y_lo", "<u4"), ("dy", "<i4"), ("kind", "<u4")])
NONE = 0xFF
A_, C_, G_, T_ = 0, 1, 2, 3


def s(text):
    return np.frombuffer(text.encode(), dtype=np.uint8)


def with_bases(a, b):
    return [(op, p, q, None if op == V.DEL else int(b[q])) for op, p, q in V.script(a, b)]


# ---- the brute force against itself and by hand

def test_columns_are_the_issue_s():
    assert assess.VARIANT_COLUMNS == V.COLUMNS
    assert "\t".join(assess.VARIANT_COLUMNS) == "block_id\tgenome_a\tcontig_a\tpos_a\tgenome_b\tcontig_b\tpos_b\torientation\ttype\tlength\tseq_a\tseq_b"


def test_script_applied_to_a_gives_b_and_has_the_distance():
    rng = np.random.default_rng(7)
    letters = s("ACGT")
    seen = set()
    for _ in range(300):
        a = letters[rng.integers(0, 4, size=int(rng.integers(1, 60)))]
        b = [c for c in a if rng.random() > 0.08]
        for _ in range(int(rng.integers(0, 4))):
            b.insert(int(rng.integers(0, len(b) + 1)), int(letters[rng.integers(0, 4)]))
        b = np.array(b if b else [a[0]], dtype=np.uint8)
        b[rng.random(b.size) < 0.05] = ord("G")
        ops = with_bases(a, b)
        seen |= {o[0] for o in ops}
        assert V.apply_script(a, ops).tobytes() == b.tobytes()
        assert len(ops) == B.levenshtein(a, b)
        assert [o[1] for o in ops] == sorted(o[1] for o in ops) and [o[2] for o in ops] == sorted(o[2] for o in ops)
    assert seen == {V.SUB, V.DEL, V.INS}


def test_canonical_script_by_hand():
    assert V.script(s("AAAC"), s("AAC")) == [(V.DEL, 0, 0)]                  # of a run that lost a base, the first base is deleted
    assert V.script(s("AAC"), s("AAAC")) == [(V.INS, 0, 0)]                  # an empty-prefix INS at (0, 0)
    assert V.script(s("AC"), s("CA")) == [(V.SUB, 0, 0), (V.SUB, 1, 1)]      # two substitutions, not DEL + INS
    assert V.script(s("ACGT"), s("ACGA")) == [(V.SUB, 3, 3)]                 # an edit at the last base
    assert V.script(s("ACGT"), s("ACG")) == [(V.DEL, 3, 3)]
    assert V.script(s("ACG"), s("ACGT")) == [(V.INS, 3, 3)]
    assert V.script(s("ACGT"), s("ACGT")) == []
    assert V.script(s("A"), s("CCA")) == [(V.INS, 0, 0), (V.INS, 0, 1)]
    assert V.op_records(5, s("AAAC"), s("AAC")) == [(5, 0, 0, V.DEL, A_, NONE)]
    assert V.op_records(2, s("ACG"), s("ACGT")) == [(2, 3, 3, V.INS, NONE, T_)]
    assert V.op_records(0, s("AC"), s("CA")) == [(0, 0, 0, V.SUB, A_, C_), (0, 1, 1, V.SUB, C_, A_)]


def test_table_by_hand():
    assert V.table(s("AC"), s("CA")).tolist() == [[0, 1, 2], [1, 1, 1], [2, 1, 2]]


# ---- variant_events / variants_table on hand-made ops

def ops_of(*rows):
    return np.array([tuple(r) + (0,) for r in rows], dtype=OP)


def segs_of(*rows):
    return np.array(list(rows), dtype=SEG)


def short(events):
    return [(e["type"], e["pos_a"], e["pos_b"], e["length"], e["seq_a"], e["seq_b"]) for e in events]


def test_runs_merge_and_interleaved_ones_do_not():
    segs = segs_of((0, 10, 50, 20, 50, 0))
    # three deleted bases of A at p = 4, 5, 6 against q = 4: one del; three inserted at q = 30, 31, 32 against p = 40: one ins
    ops = ops_of((0, 4, 4, V.DEL, A_, NONE), (0, 5, 4, V.DEL, C_, NONE), (0, 6, 4, V.DEL, G_, NONE),
                 (0, 40, 30, V.INS, NONE, T_), (0, 40, 31, V.INS, NONE, T_), (0, 40, 32, V.INS, NONE, A_))
    assert short(assess.variant_events(ops, segs, 1000, 2000, 500, False)) == [("del", 1014, 2024, 3, "ACG", "-"), ("ins", 1050, 2050, 3, "-", "TTA")]
    # DEL, INS, DEL: adjacent in the script but not one run; and a DEL whose p is not consecutive
    ops = ops_of((0, 4, 4, V.DEL, A_, NONE), (0, 5, 4, V.INS, NONE, T_), (0, 5, 5, V.DEL, C_, NONE), (0, 9, 8, V.DEL, C_, NONE))
    assert [e[0] for e in short(assess.variant_events(ops, segs, 0, 0, 500, False))] == ["del", "ins", "del", "del"]
    # the same p and q in two segments: no run across a segment's border
    segs2 = segs_of((0, 10, 5, 20, 4, 0), (0, 15, 5, 24, 4, 0))
    ops = ops_of((0, 4, 4, V.DEL, A_, NONE), (1, 0, 0, V.DEL, A_, NONE))
    assert short(assess.variant_events(ops, segs2, 0, 0, 500, False)) == [("del", 14, 24, 1, "A", "-"), ("del", 15, 24, 1, "A", "-")]
    # SUBs never merge
    ops = ops_of((0, 4, 4, V.SUB, A_, C_), (0, 5, 5, V.SUB, A_, C_))
    assert short(assess.variant_events(ops, segs, 0, 0, 500, False)) == [("snv", 14, 24, 1, "A", "C"), ("snv", 15, 25, 1, "A", "C")]


def test_coordinates_of_both_orientations_by_hand():
    # intervals: A starts at 1000, B at 2000 with 500 bases; the segment at x = 10, y_lo = 20
    segs = segs_of((0, 10, 50, 20, 50, 0))
    ops = ops_of((0, 3, 3, V.SUB, A_, G_), (0, 7, 7, V.DEL, C_, NONE), (0, 8, 7, V.DEL, C_, NONE), (0, 30, 28, V.INS, NONE, T_), (0, 30, 29, V.INS, NONE, G_))
    plus = short(assess.variant_events(ops, segs, 1000, 2000, 500, False))
    # +: pos_b = 2000 + 20 + q0
    assert plus == [("snv", 1013, 2023, 1, "A", "G"), ("del", 1017, 2027, 2, "CC", "-"), ("ins", 1040, 2048, 2, "-", "TG")]
    minus = short(assess.variant_events(ops, segs, 1000, 2000, 500, True))
    # -: y = 20 + q0; pos_b = 2000 + 500 - y - l_b: snv 2500 - 23 - 1, del 2500 - 27 - 0 (the base that follows in the oriented frame
    # is oriented offset 27 = forward 2472, so the forward position of the gap's right neighbour is 2473), ins 2500 - 48 - 2
    assert minus == [("snv", 1013, 2476, 1, "A", "G"), ("del", 1017, 2473, 2, "CC", "-"), ("ins", 1040, 2450, 2, "-", "TG")]
    for got in (plus, minus):
        for (kind, pa, pb, n, sa, sb), ev, (x, y_lo) in zip(got, V.events([(int(o["op"]), int(o["p"]), int(o["q"])) for o in ops], s("ACGA" * 13), s("TGTG" * 13)),
                                                          [(10, 20)] * 3):
            assert (pa, pb) == V.place(ev, x, y_lo, 1000, 2000, 500, got is minus)


def test_events_at_an_interval_s_first_and_last_base():
    segs = segs_of((0, 0, 40, 0, 40, 0))                      # the segment is the whole interval of 40 bases, in both genomes
    ops = ops_of((0, 0, 0, V.SUB, A_, C_), (0, 39, 39, V.SUB, G_, T_))
    assert short(assess.variant_events(ops, segs, 100, 300, 40, False)) == [("snv", 100, 300, 1, "A", "C"), ("snv", 139, 339, 1, "G", "T")]
    assert short(assess.variant_events(ops, segs, 100, 300, 40, True)) == [("snv", 100, 339, 1, "A", "C"), ("snv", 139, 300, 1, "G", "T")]
    ops = ops_of((0, 0, 0, V.INS, NONE, C_), (0, 39, 40, V.DEL, G_, NONE))
    segs = segs_of((0, 0, 40, 0, 40, 0))
    assert short(assess.variant_events(ops, segs, 100, 300, 40, True)) == [("ins", 100, 339, 1, "-", "C"), ("del", 139, 300, 1, "G", "-")]


def test_events_ascend_by_pos_a_then_script_order():
    # an INS behind the last base of one segment and a SUB at the first base of the next share pos_a: script order decides
    segs = segs_of((0, 0, 10, 0, 11, 0), (0, 10, 10, 11, 10, 0))
    ops = ops_of((0, 10, 10, V.INS, NONE, C_), (1, 0, 0, V.SUB, A_, T_))
    assert short(assess.variant_events(ops, segs, 0, 0, 100, False)) == [("ins", 10, 10, 1, "-", "C"), ("snv", 10, 11, 1, "A", "T")]


def test_what_is_no_op_is_refused():
    segs = segs_of((0, 0, 10, 0, 10, 0))
    for bad in ((0, 1, 1, 0, A_, C_), (0, 1, 1, 4, A_, C_), (0, 1, 1, V.SUB, NONE, C_), (0, 1, 1, V.INS, NONE, 4)):
        with pytest.raises(ValueError):
            assess.variant_events(ops_of(bad), segs, 0, 0, 100, False)


def test_table_footer_and_the_empty_table():
    ev = assess.variant_events(ops_of((0, 3, 3, V.SUB, A_, G_)), segs_of((0, 10, 50, 20, 50, 0)), 1000, 2000, 500, True)[0]
    r = dict(ev, block_id="7", genome_a="a.fa", contig_a="chr1", genome_b="b.fa", contig_b="chr2", orientation="-")
    assert assess.variant_row(r) == "7\ta.fa\tchr1\t1013\tb.fa\tchr2\t2476\t-\tsnv\t1\tA\tG"
    text = assess.variants_table([r, r], 21, 16, 31, 4096)
    assert text.split("\n") == ["\t".join(assess.VARIANT_COLUMNS), assess.variant_row(r), assess.variant_row(r), "# k 21, rate 16, band 31, max_len 4096", ""]
    assert assess.variants_table([], 19, 4, 7, 100) == "\t".join(assess.VARIANT_COLUMNS) + "\n# k 19, rate 4, band 7, max_len 100\n"
    assert assess.variant_events(np.zeros(0, dtype=OP), segs_of(), 0, 0, 0, False) == []


# ---- argument parsing

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
    args = parse(["a.fa", "b.fa", "-d", "1", "--block-variants"], monkeypatch)
    assert args.block_variants and not args.block_identity
    assert (args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len) == (21, 16, 31, 4096)
    assert not parse(["a.fa", "b.fa", "-d", "1", "--block-identity"], monkeypatch).block_variants
    parse(["a.fa", "b.fa", "-d", "1", "--block-variants", "--block-identity", "--identity-band", "1"], monkeypatch)
    for bad in (["--identity-band", "0"], ["--identity-band", "32"], ["--identity-max-len", "0"], ["--identity-max-len", "65536"],
                ["--identity-rate", "0"], ["--identity-k", "0"]):
        with pytest.raises(SystemExit) as err:
            parse(["a.fa", "b.fa", "-d", "1", "--block-variants"] + bad, monkeypatch)
        assert err.value.code == 2
        assert bad[0] in capsys.readouterr().err


def test_refused_under_several_ranks(monkeypatch, capsys):
    with pytest.raises(SystemExit) as err:
        parse(["a.fa", "b.fa", "-d", "1", "--block-variants"], monkeypatch, world=2)
    shown = capsys.readouterr().err
    assert err.value.code == 2 and "--block-variants works from the genomes resident on one GPU" in shown
    assert "ntsynt_block_stats" in shown and "--variants-out" in shown


def test_dry_run_lists_the_stage(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--assess", "--block-identity", "--block-variants", "--gaps"]) == 0
    assert "ntsynt_synteny -> assess -> block_identity -> block_variants -> gaps" in capsys.readouterr().out
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--block-variants"]) == 0
    out = capsys.readouterr().out
    assert "ntsynt_synteny -> block_variants" in out and "block_identity" not in out
    assert cli.main(paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--block-identity"]) == 0
    assert "block_variants" not in capsys.readouterr().out


def test_tool_refuses_bad_parameters(capsys):
    for argv in (["--tsv", "x.tsv", "--fai", "a.fai", "--variants-out", "o.tsv"],
                 ["--tsv", "x.tsv", "--fai", "a.fai", "--fastas", "a.fa", "--variants-out", "o.tsv", "--identity-band", "40"]):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
    shown = capsys.readouterr().err
    assert "--variants-out needs the genomes" in shown and "--identity-band" in shown


def test_pipeline_takes_the_argument():
    import inspect
    from ntsynt_amd import pipeline
    assert inspect.signature(pipeline.run).parameters["block_variants"].default is None

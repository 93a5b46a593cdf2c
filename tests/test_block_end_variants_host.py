"""The host side of the block end variants (ntsynt_amd/assess.py ends_events, end_variants_table, block_ends with_variants;
docs/design/04_21_block_end_variants.md), no GPU: ends_events on hand-made ops for the right and the left flank of `+` and `-` pairs --
positions, lengths, reversed sequences, the position of an empty interval, the order, the merging of runs, a bad op --, then on the
flanks of a hand-made round with an insertion, a deletion and substitutions in either flank, the device calls stood in for by
tests/extend_brute.py and tests/variants_brute.py, against the recomputation of tests/end_variants_brute.py, which works a flipped pair
in the frame of the whole record's reverse complement; the table's header and footer; argument parsing (the switch without
--block-ends, several ranks), the --dry-run line, the tool's and pipeline.run's refusals."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from ntsynt_amd.device import OP_DTYPE, TASK_DTYPE
from tests import end_variants_brute as EB
from tests import extend_brute as X
from tests import variants_brute as V
from tests.test_block_ends_host import Line, device_stand_in, dna, mutated, segments

A, C, G, T, NONE = 0, 1, 2, 3, 0xFF
SUB, DEL, INS = 1, 2, 3
# in string offsets: a substitution, a deletion of three bases, an insertion of two, a deletion of one directly behind another one
# base further on (two events: the p are not consecutive), a substitution
OPS = [(9, 5, 5, SUB, A, C, 0), (9, 10, 10, DEL, C, NONE, 0), (9, 11, 10, DEL, G, NONE, 0), (9, 12, 10, DEL, T, NONE, 0),
       (9, 20, 17, INS, NONE, A, 0), (9, 20, 18, INS, NONE, G, 0), (9, 30, 29, DEL, A, NONE, 0), (9, 32, 30, DEL, C, NONE, 0),
       (9, 40, 38, SUB, T, G, 0)]


def task(pos_a, pos_b, flags):
    t = np.zeros(1, dtype=TASK_DTYPE)
    t[0] = (pos_a, pos_b, 0, 0, 100, 100, flags, 0)
    return t[0]


def fields(events):
    return [(e["type"], e["pos_a"], e["pos_b"], e["length"], e["seq_a"], e["seq_b"]) for e in events]


def test_right_flank_of_a_plus_pair():
    "both strings forwards: positions are pos + offset, script order"
    got = assess.ends_events(np.array(OPS, dtype=OP_DTYPE), task(1000, 2000, 0), "right")
    assert fields(got) == [("snv", 1005, 2005, 1, "A", "C"), ("del", 1010, 2010, 3, "CGT", "-"), ("ins", 1020, 2017, 2, "-", "AG"),
                           ("del", 1030, 2029, 1, "A", "-"), ("del", 1032, 2030, 1, "C", "-"), ("snv", 1040, 2038, 1, "T", "G")]


def test_left_flank_of_a_plus_pair():
    "both strings backwards from the base in front of the core: intervals mirrored, sequences reversed, reverse script order"
    got = assess.ends_events(OPS, task(999, 1999, 3), "left")
    assert fields(got) == [("snv", 959, 1961, 1, "T", "G"), ("del", 967, 1970, 1, "C", "-"), ("del", 969, 1971, 1, "A", "-"),
                           ("ins", 980, 1981, 2, "-", "GA"), ("del", 987, 1990, 3, "TGC", "-"), ("snv", 994, 1994, 1, "A", "C")]
    assert [e["pos_a"] for e in got] == sorted(e["pos_a"] for e in got)


def test_right_flank_of_a_minus_pair():
    "A forwards, B backwards and complemented: B's forward interval ends at pos_b - q0; base_b is already complemented as read"
    got = assess.ends_events(OPS, task(1000, 2000, 6), "right")
    assert fields(got) == [("snv", 1005, 1995, 1, "A", "C"), ("del", 1010, 1991, 3, "CGT", "-"), ("ins", 1020, 1982, 2, "-", "AG"),
                           ("del", 1030, 1972, 1, "A", "-"), ("del", 1032, 1971, 1, "C", "-"), ("snv", 1040, 1962, 1, "T", "G")]


def test_left_flank_of_a_minus_pair():
    "A backwards, B forwards and complemented"
    got = assess.ends_events(OPS, task(999, 2001, 5), "left")
    assert fields(got) == [("snv", 959, 2039, 1, "T", "G"), ("del", 967, 2031, 1, "C", "-"), ("del", 969, 2030, 1, "A", "-"),
                           ("ins", 980, 2018, 2, "-", "GA"), ("del", 987, 2011, 3, "TGC", "-"), ("snv", 994, 2006, 1, "A", "C")]


def test_runs_merge_only_when_adjacent_in_the_string_frame():
    ins_runs = [(0, 7, 3, INS, NONE, A, 0), (0, 7, 4, INS, NONE, C, 0), (0, 7, 6, INS, NONE, G, 0), (0, 8, 7, INS, NONE, T, 0)]
    got = assess.ends_events(ins_runs, task(100, 200, 0), "right")
    assert fields(got) == [("ins", 107, 203, 2, "-", "AC"), ("ins", 107, 206, 1, "-", "G"), ("ins", 108, 207, 1, "-", "T")]
    mixed = [(0, 3, 3, DEL, A, NONE, 0), (0, 4, 3, SUB, C, G, 0), (0, 5, 4, DEL, T, NONE, 0)]
    assert [e["type"] for e in assess.ends_events(mixed, task(100, 200, 0), "right")] == ["del", "snv", "del"]
    assert assess.ends_events([], task(100, 200, 0), "left") == []


def test_a_bad_op_raises():
    for bad in ((0, 1, 1, 4, A, C, 0), (0, 1, 1, 0, A, C, 0), (0, 1, 1, SUB, NONE, C, 0), (0, 1, 1, SUB, A, NONE, 0), (0, 1, 1, DEL, 4, NONE, 0),
                (0, 1, 1, INS, NONE, 7, 0)):
        with pytest.raises(ValueError, match="not an edit op"):
            assess.ends_events([bad], task(100, 200, 0), "right")
    with pytest.raises(ValueError, match="not a flank"):
        assess.ends_events([], task(100, 200, 0), "middle")


def indel_world(seed=6):
    """test_block_ends_host's world with indels: genome A one record of 3 000 bases; the copy in genome B has 1 % substitutions, nine
    bases inserted at 200 and seven deleted at 330 (the left flank of an interval whose first aligned segment begins at 600), six
    deleted at 1 900 and eight inserted at 2 050 (the right flank behind 1 700), and unrelated sequence from 2 300 on for a while"""
    rng = np.random.default_rng(seed)
    a0 = dna(rng, 3000)
    copy = mutated(rng, a0, 0.01)
    copy[2300:2420] = dna(rng, 120)
    copy = np.concatenate([copy[:200], dna(rng, 9), copy[200:330], copy[337:1900], copy[1906:2050], dna(rng, 8), copy[2050:]])
    shift = 2                                                 # (what lies behind 337 in A lies 9 - 7 further on in the copy)
    rec_a = [a0, dna(rng, 50)]
    rec_b = [np.concatenate([dna(rng, 23), copy]), np.concatenate([dna(rng, 11), X.revcomp(copy), dna(rng, 37)])]
    iv_a = (0, 500, 2500)
    iv_b = {False: (0, 523 + shift, 2523 + shift + 2), True: (1, 11 + copy.size - 2500 - shift - 2, 11 + copy.size - 500 - shift)}
    return rec_a, rec_b, iv_a, iv_b


SEGS = [(0, 100, 200, 100, 200, 0), (0, 700, 500, 700, 500, 0)]     # (x, dx, y_lo, dy in interval offsets: aligned from 600 to 1 700 of A)


@pytest.mark.parametrize("flipped", [False, True])
def test_flanks_of_a_round_against_the_recomputation(flipped):
    rec_a, rec_b, iv_a, iv_b = indel_world()
    segs, final = segments(SEGS), np.array([3, 6], dtype=np.uint32)
    ivs_a, ivs_b = np.array([iv_a], dtype=np.uint64), np.array([iv_b[flipped]], dtype=np.uint64)
    tasks, flanks = assess.ends_tasks(segs, final, ivs_a, ivs_b, [int(flipped)], [(0, 1, 0)], [r.size for r in rec_a], [r.size for r in rec_b], 4096)
    results = device_stand_in(rec_a, rec_b, tasks, 6, 255)
    got = []
    for side in ("left", "right"):
        t = tasks[flanks[0][side]]
        a, b = X.task_strings(rec_a, rec_b, (t["rec_a"], t["pos_a"], t["n"], t["rec_b"], t["pos_b"], t["m"], t["flags"]))
        res = results[flanks[0][side]]
        ops = [op + (0,) for op in V.op_records(int(flanks[0][side]), a[:res["ext_a"]], b[:res["ext_b"]])]
        assert len(ops) == res["edits"]
        got += [(side,) + fields([e])[0] for e in assess.ends_events(np.array(ops, dtype=OP_DTYPE), t, side)]
    length_b = int(ivs_b[0][2]) - int(ivs_b[0][1])
    want, edits = EB.pair_events(rec_a[0], rec_b[int(flipped)], (500, 2000), (int(ivs_b[0][1]), length_b), flipped, list(zip(SEGS, final.tolist())),
                                 4096, 255, 6)
    want = [(side, kind, pos_a, pos_b, length, seq_a, seq_b) for side, pos_a, pos_b, kind, length, seq_a, seq_b in want]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:4]
    # what the world was made for: either flank crosses its insertion and its deletion
    for side in ("left", "right"):
        kinds = [(e[1], e[4]) for e in got if e[0] == side]   # (chance matches may split an indel of random bases into pieces)
        assert {k for k, _ in kinds} == {"snv", "ins", "del"} and sum(n for k, n in kinds if k == "ins") >= 8 and sum(n for k, n in kinds if k == "del") >= 6, kinds
        assert sum(e[4] for e in got if e[0] == side) == edits[side]
        along = [e[2] for e in got if e[0] == side]
        assert along == sorted(along)
    # applying a flank's events to A's interval gives B's oriented interval
    frame_b = X.revcomp(rec_b[1]) if flipped else rec_b[0]
    row = assess.ends_row(Line("1", "a", "c", "+"), Line("1", "b", "d", "-" if flipped else "+"), ivs_a[0], ivs_b[0], flipped, flanks[0], tasks, results,
                          4096, 255)
    for side, lo_a, hi_a in (("left", row["ext_start_a"], 600), ("right", 1700, row["ext_end_a"])):
        out, at = [], lo_a
        for _, kind, pos_a, _, length, seq_a, seq_b in [e for e in got if e[0] == side]:
            out.append(rec_a[0][at:pos_a].tobytes().decode())
            assert seq_a == "-" or rec_a[0][pos_a:pos_a + len(seq_a)].tobytes().decode() == seq_a
            out.append("" if seq_b == "-" else seq_b)
            at = pos_a + (0 if seq_a == "-" else len(seq_a))
        out.append(rec_a[0][at:hi_a].tobytes().decode())
        size = frame_b.size
        lo_b, hi_b = (size - row["ext_end_b"], size - row["ext_start_b"]) if flipped else (row["ext_start_b"], row["ext_end_b"])
        core_lo, core_hi = (lo_b + row["left_b"], hi_b - row["right_b"])
        want_b = frame_b[lo_b:core_lo] if side == "left" else frame_b[core_hi:hi_b]
        assert "".join(out) == want_b.tobytes().decode(), side


def test_table_header_and_footer():
    assert assess.END_VARIANT_COLUMNS == ("block_id", "genome_a", "contig_a", "pos_a", "genome_b", "contig_b", "pos_b", "orientation", "flank", "type",
                                          "length", "seq_a", "seq_b")
    row = {"block_id": "3", "genome_a": "a.fa", "contig_a": "chr1", "pos_a": 10, "genome_b": "b.fa", "contig_b": "chr2", "pos_b": 20, "orientation": "-",
           "flank": "left", "type": "ins", "length": 2, "seq_a": "-", "seq_b": "GA"}
    text = assess.end_variants_table([row], 21, 16, 31, 4096, 0, 1500, 255, 6)
    assert text.splitlines() == ["\t".join(assess.END_VARIANT_COLUMNS), "3\ta.fa\tchr1\t10\tb.fa\tchr2\t20\t-\tleft\tins\t2\t-\tGA",
                                 "# k 21, rate 16, band 31, max_len 4096, max_edits 0, ends_max_len 1500, ends_max_edits 255, ends_penalty 6"]
    assert text.splitlines()[-1] == assess.ends_table([], 21, 16, 31, 4096, 0, 1500, 255, 6).splitlines()[-1]
    assert assess.end_variants_table([], 21, 16, 31, 4096, 0, 1500, 255, 6).count("\n") == 2


def parse(argv, monkeypatch, world=None):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if world:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_reports(parser, args)
    return args


def test_the_switch_needs_block_ends(monkeypatch, capsys):
    base = ["a.fa", "b.fa", "-d", "1"]
    args = parse(base + ["--block-ends", "--block-end-variants"], monkeypatch)
    assert args.block_ends and args.block_end_variants
    assert not parse(base + ["--block-ends"], monkeypatch).block_end_variants
    for extra in ([], ["--block-identity"], ["--block-variants"]):
        with pytest.raises(SystemExit) as err:
            parse(base + ["--block-end-variants"] + extra, monkeypatch)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert "--block-end-variants" in said and "--block-ends" in said and "--ends-out" in said, said
    assert "--block-ends" in assess.END_VARIANTS_NEED_ENDS


def test_refused_under_several_ranks(monkeypatch, capsys):
    with pytest.raises(SystemExit) as err:
        parse(["a.fa", "b.fa", "-d", "1", "--block-ends", "--block-end-variants"], monkeypatch, world=2)
    assert err.value.code == 2
    said = capsys.readouterr().err
    assert "--block-end-variants" in said and "one rank" in said and "--end-variants-out" in said


def test_dry_run_lists_the_kernels_only_with_the_switch(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    common = paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--gaps"]
    assert cli.main(common + ["--block-ends", "--block-end-variants"]) == 0
    assert "ntsynt_synteny -> block_ends (edit_extend, edit_extend_script_plan, edit_extend_script) -> gaps" in capsys.readouterr().out
    assert cli.main(common + ["--block-ends"]) == 0
    out = capsys.readouterr().out
    assert "ntsynt_synteny -> block_ends (edit_extend) -> gaps" in out and "edit_extend_script" not in out


def test_tool_refusals(capsys):
    base = ["--tsv", "x.tsv", "--fai", "a.fai"]
    for argv, words in ((base + ["--fastas", "a.fa", "--end-variants-out", "v.tsv"], ("--end-variants-out", "--ends-out")),
                        (base + ["--end-variants-out", "v.tsv"], ("--end-variants-out", "--ends-out")),
                        (base + ["--ends-out", "e.tsv", "--end-variants-out", "v.tsv"], ("--fastas",)),
                        (base + ["--fastas", "a.fa", "--ends-out", "e.tsv", "--end-variants-out", "v.tsv", "--ends-penalty", "2"], ("--ends-penalty",))):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert all(w in said for w in words), (argv, said)


def test_pipeline_refusals():
    from ntsynt_amd import pipeline
    with pytest.raises(ValueError, match="--block-ends"):
        pipeline.run(["a.fa", "b.fa"], k=24, w=100, prefix="x", backend=object(), block_end_variants=True)    # (refused before the backend is used)
    with pytest.raises(ValueError, match="block_ends"):
        pipeline.run(["a.fa", "b.fa"], k=24, w=100, prefix="x", backend=object(), block_ends=(4096, 255, 2), block_end_variants=True)

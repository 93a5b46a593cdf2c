"""The host side of the block alignments (ntsynt_amd/assess.py alignment_pieces, alignment_ops, paf_row, paf_table;
docs/design/04_22_block_alignments.md), no GPU: tests/cigar_brute.py itself on hand cases; the chains and pieces of hand-made rounds -- a
chain broken by one segment of each kind that is not aligned, flanks on a pair's first and last chain only, a pair without an aligned
segment; a hand-made pair with real strings, `+` and `-`, whose scripts come from tests/variants_brute.py and whose CIGAR from the brute
force: every record must pass apply_cigar on the substrings its own coordinates name; the new switches' parsing, --dry-run line and
refusals."""
import numpy as np
import pytest

from ntsynt_amd import assess, cli
from ntsynt_amd.device import CIG_REVERSED, EDIT_INVALID, EDIT_NOT_CANDIDATE, EDIT_OVERBAND, EDIT_PASSED, EXTEND_DTYPE, OP_DTYPE, PIECE_DTYPE
from tests import cigar_brute as CB
from tests import extend_brute as X
from tests import identity_brute as B
from tests import variants_brute as V
from tests.test_block_end_variants_host import indel_world
from tests.test_block_ends_host import Line, device_stand_in, segments

SUB, DEL, INS = CB.SUB, CB.DEL, CB.INS


# ---- the brute force itself

def test_brute_on_hand_cases():
    entries, chains = CB.brute_cigar([(0, 5, 6, 0), (0, 3, 3, 1), (2, 2, 2, 0)], [(0, 1, 1, SUB), (0, 4, 4, INS), (1, 0, 0, SUB), (2, 0, 0, SUB), (2, 1, 1, SUB)],
                                     [0, 2, 3, 5], 3)
    assert CB.cigar_string(entries) == "1=1X2=1I3=1X" + "2X"
    assert [(c["first"], c["n_cig"]) for c in chains] == [(0, 6), (6, 0), (6, 1)]
    assert chains[0] == {"first": 0, "n_cig": 6, "eq": 6, "x": 2, "ins": 1, "del": 0, "len_a": 8, "len_b": 9}
    assert chains[1] == {"first": 6, "n_cig": 0, "eq": 0, "x": 0, "ins": 0, "del": 0, "len_a": 0, "len_b": 0}
    assert CB.brute_cigar([], [], [0], 2)[1][1]["first"] == 0
    assert CB.cigar_string([(2 ** 32 + 2) << 4 | 7]) == "4294967298="
    for bad, piece in (([(0, 2, 3, SUB)], 0), ([(1, 0, 0, SUB)], 0), ([(0, 0, 0, 5)], 0), ([(0, 4, 4, DEL)], 0), ([(0, 1, 1, DEL)], 0)):
        with pytest.raises(CB.NoScript) as err:
            CB.brute_cigar([(0, 4, 4, 0)], bad, [0, 1], 1)
        assert err.value.piece == piece


def test_apply_cigar():
    assert CB.apply_cigar("ACGTAC", "ACCTTAC", "2=1X1=1I2=") == (5, 1, 1, 0)
    assert CB.apply_cigar(b"ACGT", np.frombuffer(b"AT", dtype=np.uint8), [1 << 4 | 7, 2 << 4 | 2, 1 << 4 | 7]) == (2, 0, 0, 2)
    assert CB.apply_cigar("", "", "") == (0, 0, 0, 0)
    for target, query, cigar in (("ACGT", "ACGT", "3="), ("ACGT", "ACGA", "4="), ("ACGT", "ACGT", "3=1X"), ("ACGT", "ACGT", "2=2="), ("ACGT", "ACG", "4="),
                                 ("ACGT", "ACGT", "4=1I")):
        with pytest.raises(AssertionError):
            CB.apply_cigar(target, query, cigar)


# ---- chains and pieces of hand-made rounds

def round_of_every_kind():
    """interval 0 (line pair (10, 11)): aligned stretches broken once by each kind that is not aligned; interval 1 (pair (12, 13)): nothing
    aligned; interval 3 (pair (14, 15)): two aligned stretches; interval 2 has no pair in this round.  Segments are contiguous: each
    begins where the one in front ends."""
    rows, final, x = [], [], 50
    for kind, result in ((0, 3), (0, 0), (1, EDIT_PASSED), (0, 5), (2, EDIT_PASSED), (0, 1), (0, 2), (3, EDIT_PASSED), (0, 7), (0, EDIT_INVALID), (0, 4),
                         (0, EDIT_OVERBAND), (0, 6), (7, EDIT_NOT_CANDIDATE), (0, 8)):
        rows.append((0, x, 100, x + 5, 100 if kind != 1 else -3, kind))
        final.append(result)
        x += 100
    rows += [(1, 10, 30, 10, 30, 3), (1, 40, 30, 40, 30, 0)]
    final += [EDIT_PASSED, EDIT_OVERBAND]
    rows += [(3, 0, 40, 7, 41, 0), (3, 40, 60, 48, 58, 0)]
    final += [2, 2]
    return segments(rows), np.array(final, dtype=np.uint32), [(10, 11, 0), (12, 13, 1), (14, 15, 3)]


def test_a_chain_ends_at_every_segment_that_is_not_aligned():
    segs, final, lines = round_of_every_kind()
    pieces, source, chains = assess.alignment_pieces(segs, final, lines)
    assert pieces.dtype == PIECE_DTYPE
    want = [[0, 1], [3], [5, 6], [8], [10], [12], [14], [17, 18]]             # the segments of every chain
    assert source.tolist() == [s for c in want for s in c]
    assert pieces["chain"].tolist() == [c for c, members in enumerate(want) for _ in members]
    assert pieces["n"].tolist() == [int(segs["dx"][s]) for s in source] and pieces["m"].tolist() == [int(segs["dy"][s]) for s in source]
    assert not pieces["flags"].any()
    assert chains["line"].tolist() == [0] * 7 + [2] and chains["ch"].tolist() == [0, 1, 2, 3, 4, 5, 6, 0]
    assert chains["x0"].tolist() == [50, 350, 550, 850, 1050, 1250, 1450, 0] and chains["x1"].tolist() == [250, 450, 750, 950, 1150, 1350, 1550, 100]
    assert chains["y0"].tolist() == [55, 355, 555, 855, 1055, 1255, 1455, 7] and chains["y1"].tolist() == [255, 455, 755, 955, 1155, 1355, 1555, 106]
    nothing = assess.alignment_pieces(segs[:0], final[:0], lines)
    assert nothing[0].size == 0 and nothing[1].size == 0 and nothing[2]["line"].size == 0
    segs["x"][1] += 1
    with pytest.raises(ValueError, match="contiguous"):
        assess.alignment_pieces(segs, final, lines)


def test_flanks_on_the_first_and_the_last_chain_only():
    segs, final, lines = round_of_every_kind()
    flanks = [{"x_l": 50, "y_l": 55, "x_r": 1550, "y_r": 1555, "left": 0, "right": 1}, None, {"x_l": 0, "y_l": 7, "x_r": 100, "y_r": 106, "left": 2, "right": 3}]
    results = np.array([(20, 22, 3, 20, 22), (0, 0, 0, 9, 9), (5, 5, 0, 5, 5), (31, 30, 2, 40, 40)], dtype=EXTEND_DTYPE)
    pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
    assert source.tolist() == [-1, 0, 1, 3, 5, 6, 8, 10, 12, 14, -2, -3, 17, 18, -4]
    assert pieces["chain"].tolist() == [0, 0, 0, 1, 2, 2, 3, 4, 5, 6, 6, 7, 7, 7, 7]
    assert pieces["flags"].tolist() == [CIG_REVERSED] + [0] * 10 + [CIG_REVERSED, 0, 0, 0]
    assert (pieces["n"][0], pieces["m"][0], pieces["n"][10], pieces["m"][10], pieces["n"][14], pieces["m"][14]) == (20, 22, 0, 0, 31, 30)
    assert chains["x0"].tolist() == [30, 350, 550, 850, 1050, 1250, 1450, -5] and chains["y0"].tolist() == [33, 355, 555, 855, 1055, 1255, 1455, 2]
    assert chains["x1"].tolist() == [250, 450, 750, 950, 1150, 1350, 1550, 131] and chains["y1"].tolist() == [255, 455, 755, 955, 1155, 1355, 1555, 136]
    with pytest.raises(ValueError, match="no flanks"):
        assess.alignment_pieces(segs, final, lines, [flanks[0], None, None], results)
    with pytest.raises(ValueError, match="left flank"):
        assess.alignment_pieces(segs, final, lines, [dict(flanks[0], x_l=51)] + flanks[1:], results)


def test_ops_are_gathered_and_rebased():
    "segment 1's ops come from the second (wide) script, segment 0's and 3's from the first, the flanks' from the third"
    narrow = np.array([(0, 4, 4, SUB, 1, 2, 0), (3, 0, 0, DEL, 1, 0xFF, 0), (3, 9, 8, SUB, 0, 1, 0)], dtype=OP_DTYPE)
    wide = np.array([(1, 2, 2, INS, 0xFF, 3, 0), (1, 2, 3, INS, 0xFF, 3, 0)], dtype=OP_DTYPE)
    flank = np.array([(1, 7, 7, SUB, 2, 3, 0)], dtype=OP_DTYPE)
    ops, first = assess.alignment_ops([-2, 0, 1, 3, -1], [(narrow, [0, 1, 1, 1, 3]), (wide, [0, 0, 2, 2, 2])], (flank, [0, 0, 1]))
    assert first.dtype == np.uint64 and first.tolist() == [0, 1, 2, 4, 6, 6]
    assert [tuple(o)[:4] for o in ops.tolist()] == [(0, 7, 7, SUB), (1, 4, 4, SUB), (2, 2, 2, INS), (2, 2, 3, INS), (3, 0, 0, DEL), (3, 9, 8, SUB)]
    ops, first = assess.alignment_ops([0, 1], [(narrow[:0], [0, 0, 0])])
    assert ops.size == 0 and ops.dtype == OP_DTYPE and first.tolist() == [0, 0, 0]


# ---- a pair with real strings: pieces -> brute CIGAR -> PAF line -> apply_cigar on what the line's own coordinates name

SEGS = [(0, 100, 200, 100, 200, 0), (0, 300, 400, 300, 400, 0), (0, 700, 300, 700, 300, 0), (0, 1000, 200, 1000, 200, 0)]


@pytest.mark.parametrize("with_flanks", [False, True])
@pytest.mark.parametrize("flipped", [False, True])
def test_records_of_a_hand_made_pair_pass_apply_cigar(flipped, with_flanks):
    rec_a, rec_b, iv_a, iv_b = indel_world()
    iv_b = iv_b[flipped]
    segs = segments(SEGS)
    ivs_a, ivs_b = np.array([iv_a], dtype=np.uint64), np.array([iv_b], dtype=np.uint64)
    len_b = iv_b[2] - iv_b[1]
    strings = [B.strings_of(rec_a[0], rec_b[iv_b[0]], (iv_a[1], iv_a[2] - iv_a[1]), (iv_b[1], len_b), flipped, s) for s in SEGS]
    scripts = [V.op_records(q, a, b) for q, (a, b) in enumerate(strings)]
    final = np.array([len(s) for s in scripts], dtype=np.uint32)
    final[2] = EDIT_INVALID                                   # (the third stretch counts as not aligned: two chains)
    assert all(1 <= len(s) <= 12 for s in scripts)
    n_ops = [len(s) if d < EDIT_INVALID else 0 for s, d in zip(scripts, final)]
    seg_script = (np.array([op + (0,) for s, d in zip(scripts, final) if d < EDIT_INVALID for op in s], dtype=OP_DTYPE), np.concatenate([[0], np.cumsum(n_ops)]))
    lines = [(0, 1, 0)]
    flanks = results = flank_script = None
    if with_flanks:
        tasks, flanks = assess.ends_tasks(segs, final, ivs_a, ivs_b, [int(flipped)], lines, [r.size for r in rec_a], [r.size for r in rec_b], 4096)
        results = device_stand_in(rec_a, rec_b, tasks, 6, 255)
        flank_ops, flank_first = [], [0]
        for q, t in enumerate(tasks):
            a, b = X.task_strings(rec_a, rec_b, (t["rec_a"], t["pos_a"], t["n"], t["rec_b"], t["pos_b"], t["m"], t["flags"]))
            flank_ops += [op + (0,) for op in V.op_records(q, a[:results[q]["ext_a"]], b[:results[q]["ext_b"]])]
            flank_first.append(len(flank_ops))
        assert len(flank_ops) == int(results["edits"].sum()) and min(np.diff(flank_first)) >= 10      # (either flank crosses its indels)
        flank_script = (np.array(flank_ops, dtype=OP_DTYPE), flank_first)
    pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
    assert source.tolist() == ([-1, 0, 1, 3, -2] if with_flanks else [0, 1, 3]) and chains["ch"].tolist() == [0, 1]
    ops, first = assess.alignment_ops(source, [seg_script], flank_script)
    entries, records = CB.brute_cigar(pieces.tolist(), ops.tolist(), first, 2)
    ra, rb = Line("7", "a.fa", "chrA", "+"), Line("7", "b.fa", "chrB", "-" if flipped else "+")
    rows = [assess.paf_row(ra, rb, rec_a[0].size, rec_b[iv_b[0]].size, ivs_a[0], ivs_b[0], flipped, chains["ch"][c], [chains[f][c] for f in ("x0", "x1", "y0", "y1")],
                           records[c], entries[records[c]["first"]:records[c]["first"] + records[c]["n_cig"]]) for c in range(2)]
    text = assess.paf_table(rows)
    assert text.count("\n") == 2 and not text.startswith("#") and "#" not in text
    nm = []
    for c, line in enumerate(text.splitlines()):
        f = line.split("\t")
        assert len(f) == 18 and f[0] == "chrB" and f[5] == "chrA" and f[4] == ("-" if flipped else "+") and f[11] == "255"
        assert (int(f[1]), int(f[6])) == (rec_b[iv_b[0]].size, rec_a[0].size)
        assert [t[:5] for t in f[12:]] == list(assess.PAF_TAGS) and f[13:17] == ["bi:i:7", "tg:Z:a.fa", "qg:Z:b.fa", f"ch:i:{c}"]
        target = rec_a[0][int(f[7]):int(f[8])]
        query = rec_b[iv_b[0]][int(f[2]):int(f[3])]
        eq, x, ins, dele = CB.apply_cigar(target, X.revcomp(query) if flipped else query, f[17][5:])
        assert (int(f[9]), int(f[10]), int(f[12][5:])) == (eq, eq + x + ins + dele, x + ins + dele)
        nm.append(x + ins + dele)
    flank_edits = [int(results[flanks[0][s]]["edits"]) for s in ("left", "right")] if with_flanks else [0, 0]
    assert nm == [n_ops[0] + n_ops[1] + flank_edits[0], n_ops[3] + flank_edits[1]]
    first_row, last_row = rows[0].split("\t"), rows[1].split("\t")
    if with_flanks:                                           # the formulas agree with ext_* of the ends table
        e = assess.ends_row(ra, rb, ivs_a[0], ivs_b[0], flipped, flanks[0], tasks, results, 4096, 255)
        assert (int(first_row[7]), int(last_row[8])) == (e["ext_start_a"], e["ext_end_a"])
        assert (int(last_row[2]), int(first_row[3])) == (e["ext_start_b"], e["ext_end_b"]) if flipped else \
            (int(first_row[2]), int(last_row[3])) == (e["ext_start_b"], e["ext_end_b"])
    else:
        assert (int(first_row[7]), int(last_row[8])) == (iv_a[1] + 100, iv_a[1] + 1200)


def test_a_pair_without_an_aligned_segment_has_no_record():
    segs = segments([(0, 10, 30, 10, 30, 3), (0, 40, 30, 40, 30, 0)])
    pieces, source, chains = assess.alignment_pieces(segs, np.array([EDIT_PASSED, EDIT_OVERBAND], dtype=np.uint32), [(0, 1, 0)], [None], np.zeros(0, dtype=EXTEND_DTYPE))
    assert pieces.size == 0 and source.size == 0 and chains["line"].size == 0
    assert assess.paf_table([]) == ""


def test_cigar_texts_of_many_chains_at_once():
    entries = [17 << 4 | 7, (2 ** 32 + 2) << 4 | 8, 1 << 4 | 1, 300 << 4 | 2, 9 << 4 | 7]
    assert assess.cigar_texts(entries, [0, 1, 4, 4, 4], [1, 3, 0, 1, 0]) == ["17=", "4294967298X1I300D", "", "9=", ""]
    assert assess.cigar_texts(entries, [0, 1, 4, 4, 4], [1, 3, 0, 1, 0]) == [CB.cigar_string(entries[a:a + n]) for a, n in ((0, 1), (1, 3), (4, 0), (4, 1), (4, 0))]
    assert assess.cigar_text(np.array(entries, dtype=np.uint64)) == CB.cigar_string(entries) and assess.cigar_text([]) == ""
    assert assess.cigar_texts([], [0, 0], [0, 0]) == ["", ""]
    rng = np.random.default_rng(3)
    many = ((rng.integers(1, 2 ** 40, 5000).astype(np.uint64) >> rng.integers(0, 40, 5000).astype(np.uint64)) + np.uint64(1)) << np.uint64(4) | \
        np.array([1, 2, 7, 8], dtype=np.uint64)[rng.integers(0, 4, 5000)]
    cuts = np.sort(rng.integers(0, 5001, 99))
    first, n_cig = np.concatenate([[0], cuts]), np.diff(np.concatenate([[0], cuts, [5000]]))
    assert assess.cigar_texts(many, first, n_cig) == [CB.cigar_string(many[a:a + n].tolist()) for a, n in zip(first, n_cig)]
    with pytest.raises(ValueError, match="code"):
        assess.cigar_text([5 << 4 | 3])


# ---- the switches

def parse(argv, monkeypatch, world=None):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if world:
        monkeypatch.setenv("WORLD_SIZE", str(world))
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_reports(parser, args)
    return args


def test_the_switch_parses_alone_and_with_the_other_block_switches(monkeypatch, capsys):
    base = ["a.fa", "b.fa", "-d", "1"]
    assert parse(base + ["--block-paf"], monkeypatch).block_paf and not parse(base, monkeypatch).block_paf
    args = parse(base + ["--block-paf", "--identity-max-edits", "1023", "--block-ends", "--block-identity", "--block-wide-variants"], monkeypatch)
    assert args.block_paf and args.block_ends and args.identity_max_edits == 1023
    for extra, word in ((["--identity-band", "32"], "--identity-band"), (["--identity-max-edits", "40"], "--identity-max-edits"),
                        (["--block-ends", "--ends-penalty", "2"], "--ends-penalty")):
        with pytest.raises(SystemExit) as err:
            parse(base + ["--block-paf"] + extra, monkeypatch)
        assert err.value.code == 2 and word in capsys.readouterr().err


def test_refused_under_several_ranks(monkeypatch, capsys):
    with pytest.raises(SystemExit) as err:
        parse(["a.fa", "b.fa", "-d", "1", "--block-paf"], monkeypatch, world=2)
    assert err.value.code == 2
    said = capsys.readouterr().err
    assert "--block-paf" in said and "one rank" in said and "--paf-out" in said


def test_dry_run_lists_the_stage_and_its_parameters(monkeypatch, capsys, tmp_path):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">chr1\nACGT\n")
    common = paths + ["-d", "1", "-p", str(tmp_path / "run"), "--dry-run", "--gaps"]
    assert cli.main(common + ["--block-ends", "--block-paf", "--identity-max-edits", "1023"]) == 0
    assert ("block_ends (edit_extend) -> block_paf (cigar_atoms, cigar_merge; k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 4096, "
            "ends_max_edits 255, ends_penalty 6) -> gaps") in capsys.readouterr().out
    assert cli.main(common + ["--block-paf"]) == 0
    assert "ntsynt_synteny -> block_paf (cigar_atoms, cigar_merge; k 21, rate 16, band 31, max_len 4096, max_edits 0) -> gaps" in capsys.readouterr().out
    assert cli.main(common) == 0
    assert "paf" not in capsys.readouterr().out


def test_tool_refusals(capsys):
    base = ["--tsv", "x.tsv", "--fai", "a.fai"]
    for argv, words in ((base + ["--paf-out", "x.paf"], ("--paf-out", "--fastas")),
                        (base + ["--fastas", "a.fa", "--paf-out", "x.paf", "--identity-max-edits", "7"], ("--identity-max-edits",)),
                        (base + ["--fastas", "a.fa", "--paf-out", "x.paf", "--ends-out", "e.tsv", "--ends-max-edits", "0"], ("--ends-max-edits",))):
        with pytest.raises(SystemExit) as err:
            assess.main(argv)
        assert err.value.code == 2
        said = capsys.readouterr().err
        assert all(w in said for w in words), (argv, said)


def test_pipeline_and_library_refusals():
    from ntsynt_amd import pipeline
    for bad, word in (((21, 16, 31, 4096, 0), "block_paf ="), ((21, 16, 32, 4096, 0, None), "--identity-band"), ((21, 16, 31, 4096, 0, (4096, 255)), "block_paf ="),
                      ((21, 16, 31, 4096, 0, (4096, 255, 2)), "--ends-penalty")):
        with pytest.raises(ValueError, match=word):
            pipeline.run(["a.fa", "b.fa"], k=24, w=100, prefix="x", backend=object(), block_paf=bad)          # (refused before the backend is used)
    with pytest.raises(ValueError, match="--identity-max-edits"):
        assess.block_alignments(None, {}, [], max_edits=5)
    with pytest.raises(ValueError, match="--ends-max-len"):
        assess.block_alignments(None, {}, [], ends=(0, 255, 6))

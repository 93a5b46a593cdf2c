"""The host side of the joined lift (ntsynt_amd/assess.py lift_pair_ranges, _Lifter(joined=...), lift_joined_table;
docs/design/04_27_lift_joined.md) on the CPU: `+` and `-` pairs, either line as the source, intervals in front of, between, behind and
across 1, 2 and 3 chains.  The device call is replaced by the brute force (tests/lift_pairs_brute.PairWalker over the call's own
arguments); the table is checked against a second walk that starts from the PAF lines of the same chains and knows nothing of links,
ranges or oriented offsets (lift_pairs_brute.joined_from_paf)."""
from types import SimpleNamespace

import numpy as np
import pytest

from ntsynt_amd import assess as A
from ntsynt_amd.device import PAIR_RANGE_DTYPE, PAIR_STATS_DTYPE
from tests import lift_brute as LB
from tests import lift_pairs_brute as PB
from tests.test_gpu_cigar_lift import arrays

# a pair's chains: (CIGAR, open A bases in front of it, open B bases in front of it); the first one's: where it starts inside the intervals
CHAINS_3 = [("5=1X3I2D4=", 6, 9), ("3D2I6=", 40, 0), ("4=2I1X", 3, 7)]
CHAINS_2 = [("2I6=", 0, 4), ("2=2D2D1X", 0, 5)]
CHAINS_1 = [("7=", 11, 2)]


class BruteContext:
    "Context.cigar_lift_pairs by the brute force, and the calls it was given"

    def __init__(self):
        self.calls = []

    def cigar_lift_pairs(self, cigar, chains, links, pair_first, ranges):
        assert ranges.dtype == PAIR_RANGE_DTYPE and np.all(ranges["lo"] < ranges["hi"])
        self.calls.append((links.copy(), np.asarray(pair_first).copy(), ranges.copy()))
        out = np.zeros(ranges.size, dtype=PAIR_STATS_DTYPE)
        walkers = {}
        for g, (p, side, lo, hi) in enumerate(ranges.tolist()):
            if p not in walkers:
                mine = links[int(pair_first[p]):int(pair_first[p + 1])]
                walkers[p] = PB.PairWalker([(cigar[int(chains[c]["first"]):int(chains[c]["first"] + chains[c]["n_cig"])].tolist(), int(a0), int(b0))
                                            for c, _, a0, b0 in mine.tolist()], int(pair_first[p]))
            for f, v in zip(PB.FIELDS, walkers[p].stats(side, lo, hi)):
                out[f][g] = v
        return out


def make_round(name_a, name_b, pairs):
    """a round of the alignment pass as _Lifter.add_round reads it.  pairs: [(block line a, block line b, flipped, (rec, start, end) of a, of b, chains)];
    the chain records are laid out in a shuffled order, one chain without entries among them"""
    texts, line, ch, x0, x1, y0, y1 = [], [], [], [], [], [], []
    lines, iv_a, iv_b, flip = [], [], [], []
    for q, (la, lb, flipped, a, b, chains) in enumerate(pairs):
        lines.append((la, lb, q))
        iv_a.append(a)
        iv_b.append(b)
        flip.append(int(flipped))
        x = y = 0
        for number, (text, da, db) in enumerate(chains):
            entries = LB.parse_cigar(text)
            _, len_a, len_b = LB.columns(entries)
            x, y = x + da, y + db
            texts.append(entries)
            line.append(q), ch.append(number), x0.append(x), x1.append(x + len_a), y0.append(y), y1.append(y + len_b)
            x, y = x + len_a, y + len_b
    order = np.random.default_rng(3).permutation(len(texts))
    cigar, records, _ = arrays([texts[i] for i in order.tolist()] + [[]])
    chains = {f: np.array(v, dtype=np.int64)[order] for f, v in (("line", line), ("ch", ch), ("x0", x0), ("x1", x1), ("y0", y0), ("y1", y1))}
    chains = {f: np.append(v, [0 if f == "line" else 9 if f == "ch" else 1]) for f, v in chains.items()}      # the empty chain: pair 0, offsets 1 .. 1
    names = ["c0", "c1"]
    r = SimpleNamespace(name_a=name_a, name_b=name_b, g_a=SimpleNamespace(names=names, rec_len=[10_000, 10_000]), g_b=SimpleNamespace(names=names, rec_len=[10_000, 10_000]),
                        lines=lines, iv_a=np.array(iv_a, dtype=np.int64), iv_b=np.array(iv_b, dtype=np.int64), flip=np.array(flip, dtype=np.int64))
    return SimpleNamespace(round=r, chains=chains, cigar=cigar, records=records)


def world():
    blocks = [A.BlockRow("7", "g0", "c0", 100, 400, "+", "", ""), A.BlockRow("7", "g1", "c1", 1000, 1300, "-", "", ""),
              A.BlockRow("8", "g0", "c1", 50, 300, "+", "", ""), A.BlockRow("8", "g1", "c0", 500, 700, "+", "", ""),
              A.BlockRow("9", "g0", "c0", 600, 700, "+", "", ""), A.BlockRow("9", "g1", "c0", 20, 90, "-", "", "")]
    pairs = [(0, 1, True, (0, 100, 400), (1, 1000, 1300), CHAINS_3), (2, 3, False, (1, 50, 300), (0, 500, 700), CHAINS_2),
             (4, 5, True, (0, 600, 700), (0, 20, 90), CHAINS_1)]
    return blocks, make_round("g0", "g1", pairs), [(0, 1), (2, 3), (4, 5)]


def paf_of(blocks, a):
    "the PAF lines of the round's chains with entries (assess.paf_row), pairs in order, chains ascending by ch"
    r, out = a.round, []
    for q, (la, lb, i) in enumerate(r.lines):
        mine = [c for c in np.flatnonzero(a.chains["line"] == q).tolist() if int(a.records[c]["n_cig"])]
        for c in sorted(mine, key=lambda c: int(a.chains["ch"][c])):
            rec = a.records[c]
            out.append(A.paf_row(blocks[la], blocks[lb], 10_000, 10_000, r.iv_a[i], r.iv_b[i], bool(r.flip[i]), a.chains["ch"][c],
                                 [a.chains[f][c] for f in ("x0", "x1", "y0", "y1")], rec, a.cigar[int(rec["first"]):int(rec["first"] + rec["n_cig"])]))
    return "\n".join(out) + "\n"


def intervals_on(blocks, a, source):
    "intervals in front of, between, behind and across the chains of every pair, on the forward strand of `source`, and some elsewhere"
    side = 0 if a.round.name_a == source else 1
    bed = []
    for line in paf_of(blocks, a).splitlines():
        f = line.split("\t")
        contig, s0, s1 = (f[0], int(f[2]), int(f[3])) if side else (f[5], int(f[7]), int(f[8]))
        bed += [(contig, s0 - 3, s0), (contig, s0 - 2, s0 + 1), (contig, s0, s1), (contig, s0 + 1, s1 - 1), (contig, s1 - 1, s1 + 2), (contig, s1, s1 + 4),
                (contig, max(s0 - 60, 0), s1 + 60), (contig, s0 + 2, s1 + 45), (contig, max(s0 - 45, 0), s0 + 3)]
    bed += [("c0", 0, 10_000), ("c1", 0, 10_000), ("c1", 9_000, 9_001), ("c0", 9_000, 9_001)]
    bed = [(c, s, e, f"iv{n}") for n, (c, s, e) in enumerate(dict.fromkeys(bed)) if 0 <= s < e]
    return bed, {"contig": [b[0] for b in bed], "name": [b[3] for b in bed], "start": np.array([b[1] for b in bed], dtype=np.int64),
                 "end": np.array([b[2] for b in bed], dtype=np.int64)}


@pytest.mark.parametrize("source", ["g0", "g1"])
def test_the_joined_table_against_a_walk_over_the_paf(source):
    blocks, a, pairs = world()
    bed, intervals = intervals_on(blocks, a, source)
    ctx = BruteContext()
    lifter = A._Lifter({"g0": None, "g1": None}, blocks, source, intervals, joined=np.ones(len(bed), dtype=bool), per_chain=False)
    lifter.add_round(ctx, a, pairs)
    rows = lifter.joined_rows({"g0": None, "g1": None})
    text = A.lift_joined_table(rows, 15, 1, 15, 1000)
    lines = text.splitlines()
    assert lines[0].split("\t") == list(A.LIFT_JOINED_COLUMNS) and lines[-1].startswith("# k 15, rate 1, band 15, max_len 1000, max_edits 0")
    want = PB.joined_from_paf(paf_of(blocks, a), bed, source)
    assert lines[1:-1] == want, [(h, w) for h, w in zip(lines[1:-1], want) if h != w][:2]
    by_status = {s: sum(l.endswith("\t" + s) for l in want) for s in ("full", "partial", "unmapped")}
    assert min(by_status.values()) >= 3, by_status
    chains = sorted({int(l.split("\t")[11]) for l in want if not l.endswith("unmapped")})
    assert chains == [1, 2, 3] and any(l.split("\t")[10] == "-" for l in want) and any(l.split("\t")[10] == "+" for l in want)
    assert any(int(l.split("\t")[22]) > 0 for l in want if not l.endswith("unmapped"))       # open bases between two chains
    # ONE call for the round; the chain without entries is not linked; every range reaches its pair's hull
    assert len(ctx.calls) == 1
    links, pair_first, ranges = ctx.calls[0]
    assert links.size == 6 and pair_first.tolist() == [0, 3, 5, 6] and np.all(a.records["n_cig"][links["chain"]] > 0)
    assert set(ranges["side"].tolist()) == {0 if source == "g0" else 1}


def test_lift_pair_ranges_mirrors_side_b_of_a_minus_pair():
    pairs = {"side": [1, 1, 0], "flip": [True, False, True], "contig": ["c1", "c0", "c0"], "origin": [1300, 500, 100], "h0": [9, 4, 6], "h1": [80, 30, 70]}
    iv = {"contig": ["c1", "c1", "c1", "c0", "c0", "c0", "c0", "c2"], "name": ["."] * 8,
          "start": np.array([1200, 1291, 1220, 0, 504, 530, 100, 0]), "end": np.array([1220, 1300, 1221, 10_000, 505, 531, 106, 5])}
    ranges, which = A.lift_pair_ranges(pairs, iv)
    got = sorted(zip(which.tolist(), ranges["pair"].tolist(), ranges["side"].tolist(), ranges["lo"].tolist(), ranges["hi"].tolist()))
    # pair 0: forward hull 1220 .. 1291 on c1, offsets run backwards from 1300; pair 1: 504 .. 530 on c0; pair 2: 106 .. 170 on c0
    assert got == [(2, 0, 1, 79, 80), (3, 1, 1, 4, 30), (3, 2, 0, 6, 70), (4, 1, 1, 4, 5)]
    none = A.lift_pair_ranges({"side": [], "flip": [], "contig": [], "origin": [], "h0": [], "h1": []}, iv)
    assert none[0].size == 0 and none[1].size == 0 and none[0].dtype == PAIR_RANGE_DTYPE


def test_a_flank_that_leaves_the_interval_moves_the_links_not_the_answer():
    "offsets in front of the interval's start are negative: the pair's links are moved so that none is, and the table does not change"
    blocks = [A.BlockRow("1", "g0", "c0", 100, 200, "+", "", ""), A.BlockRow("1", "g1", "c1", 300, 400, "-", "", "")]
    a = make_round("g0", "g1", [(0, 1, True, (0, 100, 200), (1, 300, 400), [("4=1X2=", 0, 0), ("3=2D1=", 5, 2)])])
    a.chains["x0"][a.chains["ch"] < 9] -= 3
    a.chains["x1"][a.chains["ch"] < 9] -= 3
    a.chains["y0"][a.chains["ch"] < 9] -= 2
    a.chains["y1"][a.chains["ch"] < 9] -= 2
    for source in ("g0", "g1"):
        bed, intervals = intervals_on(blocks, a, source)
        ctx = BruteContext()
        lifter = A._Lifter({"g0": None, "g1": None}, blocks, source, intervals, joined=np.ones(len(bed), dtype=bool), per_chain=False)
        lifter.add_round(ctx, a, [(0, 1)])
        lines = A.lift_joined_table(lifter.joined_rows({"g0": None, "g1": None}), 15, 1, 15, 1000).splitlines()[1:-1]
        assert lines == PB.joined_from_paf(paf_of(blocks, a), bed, source)
        assert int(ctx.calls[0][0]["a0"].min()) == 0 and int(ctx.calls[0][0]["b0"].min()) == 0


@pytest.fixture()
def fastas(tmp_path):
    paths = []
    for name in ("one.fa", "two.fa"):
        (tmp_path / name).write_text(">chr1\nACGT\n")
        paths.append(str(tmp_path / name))
    return paths


def stopped(main, argv, capsys, monkeypatch, **env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    with pytest.raises(SystemExit) as stop:
        main(argv)
    assert stop.value.code == 2
    return capsys.readouterr().err


def test_the_parser_rules_of_ntsynt_and_the_dry_run(fastas, capsys, monkeypatch):
    from ntsynt_amd import cli
    base = fastas + ["-d", "1"]
    assert "--lift-join joins the lines of --block-lift BED and/or --lift-windows W" in stopped(cli.main, base + ["--lift-join"], capsys, monkeypatch)
    tail = "k 21, rate 16, band 31, max_len 4096, max_edits 0)"
    assert cli.main(base + ["--dry-run", "--block-lift", "x.bed", "--lift-genome", "one.fa", "--lift-windows", "1000", "--lift-join", "--gaps"]) == 0
    out = capsys.readouterr().out
    assert f"block_windows (lift_stats_scan, lift_stats_search; windows of 1000 on one.fa; {tail} -> block_lift_joined (lift_pairs_scan, lift_pairs_search; "\
           f"x.bed and windows of 1000 on one.fa; {tail} -> gaps" in out, out
    assert cli.main(base + ["--dry-run", "--lift-windows", "500", "--lift-genome", "two.fa", "--lift-join"]) == 0
    assert capsys.readouterr().out.rstrip().endswith(f"-> block_lift_joined (lift_pairs_scan, lift_pairs_search; windows of 500 on two.fa; {tail}")
    assert cli.main(base + ["--dry-run", "--lift-windows", "500", "--lift-genome", "two.fa"]) == 0       # (the switch off: no word of it)
    out = capsys.readouterr().out
    assert "joined" not in out and "lift_pairs" not in out
    err = stopped(cli.main, base + ["--block-lift", "x.bed", "--lift-genome", "one.fa", "--lift-join"], capsys, monkeypatch, WORLD_SIZE="2", RANK="0")
    assert "--lift-join works from the genomes resident on one GPU" in err and "ntsynt_block_stats --tsv" in err and "--lift-joined-out" in err


def test_the_parser_rules_of_the_tool(tmp_path, capsys, monkeypatch):
    tsv, fai = tmp_path / "b.tsv", tmp_path / "one.fa.fai"
    tsv.write_text("0\tone.fa\tchr1\t0\t4\t+\t2\t\n")
    fai.write_text("chr1\t4\t6\t4\t5\n")
    base = ["--tsv", str(tsv), "--fai", str(fai)]
    assert "--lift-joined-out needs the intervals and their genome" in stopped(A.main, base + ["--lift-joined-out", "j.tsv"], capsys, monkeypatch)
    assert "--lift-joined-out needs the intervals and their genome" in stopped(A.main, base + ["--lift-joined-out", "j.tsv", "--lift-bed", "x.bed"], capsys, monkeypatch)
    assert "--lift-windows-joined-out needs the windows" in stopped(A.main, base + ["--lift-windows-joined-out", "j.tsv", "--lift-genome", "one.fa"], capsys, monkeypatch)
    assert "--lift-windows and --lift-windows-out go together" in stopped(A.main, base + ["--lift-windows", "10", "--lift-genome", "one.fa"], capsys, monkeypatch)
    assert "needs the genomes: --fastas" in stopped(A.main, base + ["--lift-joined-out", "j.tsv", "--lift-bed", "x.bed", "--lift-genome", "one.fa"], capsys, monkeypatch)


def test_the_pipeline_takes_the_argument():
    from ntsynt_amd import pipeline
    import inspect
    assert "block_lift_joined" in inspect.signature(pipeline.run).parameters

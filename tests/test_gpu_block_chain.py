"""`ntSynt --block-chain` and `bin/ntsynt_block_stats --chain-out` end to end (ntsynt_amd/assess.py block_chains, chain_table;
docs/design/04_28_block_chain.md) on the family of tests/test_gpu_block_paf.py.  Every file passes the strict reader and equals
tests/chain_brute.chains_from_paf of the same run's PAF; every block's target and query substrings, read from the FASTA files (the query
reverse-complemented for `-`), have the block's length and differ in exactly as many places as the PAF has X columns inside it, and the
scores are the PAF's matches per pair; with E = 0 and without ends liftOver's per-base rule through the file agrees with
block_lift_joined.tsv at the first and last base of every `full` line, and the planted 40-base deletion is a gap line inside ONE
liftover chain; with E = 1023 and ends every pair is one liftover chain over ext_start_a .. ext_end_a; --block-paf and --block-chain
together give the files each gives alone; the tool reproduces the file; every other file is that of the run without the switch.  In
front of these, the host path on the fabricated round of tests/test_chain_host.py: ONE nts_cigar_chain_blocks per round, `-` pairs on
the query's reverse strand, a pair without a match column left out.  Every test runs under a time limit of its own."""
import faulthandler

import os
import sys

import numpy as np
import pytest

from ntsynt_amd import assess
from tests import chain_brute as CB
from tests import extend_brute as X
from tests.test_chain_host import ROUND_PAIRS, fabricated_round
from tests.test_gpu_block_lift import NTSYNT, ROOT, _run
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, PARAMS, SWITCHES, paf_family, read_fasta, tsv_rows

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
SOURCE = "fam0.fa"
CHAIN, PAF = "g.block_alignments.chain", "g.block_alignments.paf"


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def made():
    from ntsynt_amd.device import Context
    blocks, a = fabricated_round()
    ctx = Context(0)
    ctx.profile(True)
    try:
        before = [ctx.timing(t)[1] for t in ("chain_blocks_scan", "chain_blocks_emit", "chain_text")]
        found, chains_of = {}, {}
        assess._round_paf_rows(blocks, a, found)
        assess._round_chain_parts(ctx, blocks, a, chains_of)
        after = [ctx.timing(t)[1] for t in ("chain_blocks_scan", "chain_blocks_emit", "chain_text")]
    finally:
        ctx.close()
    pairs = [(la, lb) for la, lb, _ in a.round.lines]
    paf = assess.paf_table([row for p in pairs for row in found[p]])
    text = assess.chain_table([chains_of[p] for p in pairs if chains_of[p] is not None])
    return a, paf, text, chains_of, (before, after)


def test_one_call_per_round_and_a_file_the_strict_reader_accepts(made):
    a, _, text, chains_of, (before, after) = made
    assert [y - x for x, y in zip(before, after)] == [1, 1, 2]          # one call: the byte scan and the text kernel each under chain_text
    chains = CB.parse_chain(text)
    assert len(chains) == 4 and chains_of[(4, 5)] is None and [c["id"] for c in chains] == [1, 2, 3, 4]
    assert [c["qStrand"] for c in chains] == ["-" if f else "+" for q, (f, _) in enumerate(ROUND_PAIRS) if q != 2]


def test_the_file_equals_the_one_built_from_the_paf_alone(made):
    _, paf, text, _, _ = made
    want = CB.chains_from_paf(paf)
    assert text == want, [(g, w) for g, w in zip(text.splitlines(), want.splitlines()) if g != w][:3]


def test_scores_and_first_and_last_bases_against_the_paf(made):
    _, paf, text, _, _ = made
    chains = {c["tName"]: c for c in CB.parse_chain(text)}
    matches, first, last = {}, {}, {}
    # (the fabricated round holds its chain records in a random order, so a pair's rows are ordered by their ch tag here)
    for f in sorted((line.split("\t") for line in paf.splitlines()), key=lambda f: (f[5], int(f[16][5:]))):
        entries = CB.LB.parse_cigar(f[-1][5:])
        if not any(v & 15 in (CB.EQ, CB.X) for v in entries):
            continue
        matches[f[5]] = matches.get(f[5], 0) + int(f[9])
        first.setdefault(f[5], (f, entries))
        last[f[5]] = (f, entries)
    assert {t: c["score"] for t, c in chains.items()} == matches
    for t, c in chains.items():
        # the first match column of the pair's first record with one: behind the record's leading gaps
        f, entries = first[t]
        lead_a = lead_b = 0
        for v in entries:
            if v & 15 in (CB.EQ, CB.X):
                break
            lead_a, lead_b = lead_a + (v >> 4 if v & 15 == CB.D else 0), lead_b + (v >> 4 if v & 15 == CB.I else 0)
        q_forward = int(f[3]) - 1 - lead_b if f[4] == "-" else int(f[2]) + lead_b
        assert c["tStart"] == int(f[7]) + lead_a and CB.lift_base(chains.values(), t, c["tStart"]) == [(f[0], f[4], q_forward)]
        f, entries = last[t]
        tail_a = tail_b = 0
        for v in reversed(entries):
            if v & 15 in (CB.EQ, CB.X):
                break
            tail_a, tail_b = tail_a + (v >> 4 if v & 15 == CB.D else 0), tail_b + (v >> 4 if v & 15 == CB.I else 0)
        q_forward = int(f[2]) + tail_b if f[4] == "-" else int(f[3]) - 1 - tail_b
        assert c["tEnd"] == int(f[8]) - tail_a and CB.lift_base(chains.values(), t, c["tEnd"] - 1) == [(f[0], f[4], q_forward)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 0 without ends with the joined lift (with and without the switch), each switch alone, both, and E = 1023 with ends"
    tmp = tmp_path_factory.mktemp("chain_runs")
    paths, fam = paf_family(str(tmp))
    bed = [("chr1", 5_000, 5_100, "inside"), ("chr1", 40_000, 40_250, "inside"), ("chr2", 10_000, 10_100, "inside"), ("chr1", 49_900, 50_200, "across_deletion"),
           ("chr1", 44_800, 45_200, "across_insertion"), ("chr2", 27_950, 28_050, "inversion_border"), ("chr1", 11_000, 51_000, "long")] + \
        [("chr1", s, s + 300, f"grid{s}") for s in range(1_000, 58_000, 1_700)] + [("chr2", s, s + 300, f"grid{s}") for s in range(1_000, 55_000, 1_900)]
    (tmp / "iv.bed").write_text("".join("\t".join(str(v) for v in b) + "\n" for b in bed))
    lift = ["--block-paf", "--benchmark", "--block-lift", str(tmp / "iv.bed"), "--lift-genome", SOURCE, "--lift-join"]
    dirs = {}
    for key, switches in (("without", lift), ("narrow", lift + ["--block-chain"]), ("paf_alone", ["--block-paf"]), ("chain_alone", ["--block-chain"]),
                          ("both", ["--block-paf", "--block-chain"]), ("full", SWITCHES + ["--block-paf", "--block-chain"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def pairs_of(paf_text):
    "the pairs of a PAF text with a match column, in file order: (bi, tg, qg, `-`?, the target positions of its X columns)"
    groups = {}
    for line in paf_text.splitlines():
        f = line.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        g = groups.setdefault((tags["bi:i:"], tags["tg:Z:"], tags["qg:Z:"]), dict(flip=f[4] == "-", x=set(), eq=0, match=False))
        at = int(f[7])
        for v in CB.LB.parse_cigar(tags["cg:Z:"]):
            code, n = v & 15, v >> 4
            if code == CB.X:
                g["x"].update(range(at, at + n))
            g["match"] = g["match"] or code in (CB.EQ, CB.X)
            at += n if code in (CB.EQ, CB.X, CB.D) else 0
        g["eq"] += int(f[9])
    return [(key, g) for key, g in groups.items() if g["match"]]


def test_every_file_passes_the_reader_and_equals_the_one_built_from_its_paf(runs):
    _, _, dirs = runs
    for key in ("narrow", "both", "full"):
        text, paf = (dirs[key] / CHAIN).read_text(), (dirs[key] / PAF).read_text()
        chains = CB.parse_chain(text)
        want = CB.chains_from_paf(paf)
        print(key, len(chains), "liftover chains,", sum(len(c["blocks"]) for c in chains), "blocks,", len(paf.splitlines()), "PAF records")
        assert len(chains) >= 6 and {c["qStrand"] for c in chains} == {"+", "-"}
        assert text == want, [(g, w) for g, w in zip(text.splitlines(), want.splitlines()) if g != w][:3]


def test_every_block_against_the_fasta_files_and_the_scores_against_the_paf(runs):
    _, paths, dirs = runs
    genomes = {os.path.basename(p): read_fasta(p) for p in paths}
    for key in ("narrow", "full"):
        chains, pairs = CB.parse_chain((dirs[key] / CHAIN).read_text()), pairs_of((dirs[key] / PAF).read_text())
        assert len(chains) == len(pairs)
        mismatches = 0
        for c, ((_, tg, qg), g) in zip(chains, pairs):
            target, query = genomes[tg][c["tName"]], genomes[qg][c["qName"]]
            assert (c["tSize"], c["qSize"], c["qStrand"] == "-", c["score"]) == (target.size, query.size, g["flip"], g["eq"]), c["id"]
            query = X.revcomp(query) if g["flip"] else query
            for t, q, size in CB.chain_blocks(c):
                a, b = target[t:t + size], query[q:q + size]
                assert a.size == b.size == size
                differ = int(np.count_nonzero(a != b))
                assert differ == sum(1 for pos in range(t, t + size) if pos in g["x"]), (key, c["id"], t, q, size)
                mismatches += differ
        assert mismatches > 100


def narrow_chains(dirs):
    chains, pairs = CB.parse_chain((dirs["narrow"] / CHAIN).read_text()), pairs_of((dirs["narrow"] / PAF).read_text())
    return [(key, c) for c, (key, _) in zip(chains, pairs)]


def test_lift_base_agrees_with_the_joined_lift_at_both_ends_of_every_full_line(runs):
    _, _, dirs = runs
    lines = (dirs["narrow"] / "g.block_lift_joined.tsv").read_text().splitlines()
    rows = [dict(zip(assess.LIFT_JOINED_COLUMNS, ln.split("\t"))) for ln in lines[1:-1]]
    keyed = narrow_chains(dirs)
    checked = in_gap = 0
    for r in rows:
        mine = [c for (block, tg, qg), c in keyed if (block, tg, qg) == (r["block_id"], SOURCE, r["to_genome"])]
        if r["status"] != "full" or not mine:                # (the chain file lifts from a pair's first genome: the pairs whose target is SOURCE)
            continue
        flip = r["orientation"] == "-"
        for pos, want in ((int(r["start"]), int(r["to_end"]) - 1 if flip else int(r["to_start"])),
                          (int(r["end"]) - 1, int(r["to_start"]) if flip else int(r["to_end"]) - 1)):
            got = CB.lift_base(mine, r["contig"], pos)
            if not got:                                       # the base lies in a gap line: the joined line counts bases the other genome lacks
                assert int(r["src_gap_bases"]) + int(r["src_open_bases"]) > 0, r
                in_gap += 1
                continue
            assert got == [(r["to_contig"], r["orientation"], want)], (r, pos, got)
            checked += 1
    print(checked, "ends checked,", in_gap, "in a gap")
    assert checked > 60 and checked > 10 * in_gap and any(r["orientation"] == "-" and r["status"] == "full" for r in rows)


def test_the_planted_deletion_is_a_gap_line_inside_one_liftover_chain(runs):
    _, _, dirs = runs
    holding = [c for (_, tg, qg), c in narrow_chains(dirs) if (tg, qg, c["tName"]) == (SOURCE, "fam2.fa", "chr1") and c["tStart"] <= 50_020 < c["tEnd"]]
    assert len(holding) == 1
    c = holding[0]
    assert CB.lift_base([c], "chr1", 50_020) == []            # no block holds the deleted base
    gaps = [(t + s, dt, dq) for (t, _, s), (_, dt, dq) in zip(CB.chain_blocks(c), c["blocks"]) if t + s <= 50_020 < t + s + dt]
    assert len(gaps) == 1 and gaps[0][1] - gaps[0][2] == 40, gaps
    paf = [ln.split("\t") for ln in (dirs["narrow"] / PAF).read_text().splitlines()]
    mine = [f for f in paf if f[5] == "chr1" and f[14] == "tg:Z:" + SOURCE and f[15] == "qg:Z:fam2.fa" and c["tStart"] <= int(f[7]) < c["tEnd"]]
    assert len(mine) >= 3                                     # (E = 0: several PAF records, ONE liftover chain)


def test_with_the_wide_pass_and_ends_every_pair_is_one_chain_over_its_extended_span(runs):
    _, _, dirs = runs
    chains, pairs = CB.parse_chain((dirs["full"] / CHAIN).read_text()), pairs_of((dirs["full"] / PAF).read_text())
    ends = {(r["block_id"], r["genome_a"], r["genome_b"]): r for r in tsv_rows((dirs["full"] / "g.block_ends.tsv").read_text())}
    assert len(chains) == len(pairs) >= 6
    for c, (key, _) in zip(chains, pairs):
        assert (c["tStart"], c["tEnd"]) == (int(ends[key]["ext_start_a"]), int(ends[key]["ext_end_a"])), key
        lo, hi = (c["qSize"] - c["qEnd"], c["qSize"] - c["qStart"]) if c["qStrand"] == "-" else (c["qStart"], c["qEnd"])
        assert (lo, hi) == (int(ends[key]["ext_start_b"]), int(ends[key]["ext_end_b"])), key


def test_both_switches_give_the_files_each_gives_alone(runs):
    _, _, dirs = runs
    assert (dirs["both"] / CHAIN).read_bytes() == (dirs["chain_alone"] / CHAIN).read_bytes()
    assert (dirs["both"] / PAF).read_bytes() == (dirs["paf_alone"] / PAF).read_bytes()
    assert (dirs["narrow"] / CHAIN).read_bytes() == (dirs["both"] / CHAIN).read_bytes()              # (the pass of the joined lift makes the same file)
    assert not (dirs["chain_alone"] / PAF).exists() and not (dirs["paf_alone"] / CHAIN).exists()


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    out, paf_out, alone = tmp / "tool.chain", tmp / "tool.paf", tmp / "tool_alone.chain"
    r = _run(tool + ["--chain-out", str(out), "--paf-out", str(paf_out), "--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.ends.tsv"),
                     "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_bytes() == (dirs["full"] / CHAIN).read_bytes() and paf_out.read_bytes() == (dirs["full"] / PAF).read_bytes()
    r = _run(tool + ["--chain-out", str(alone), "--divergence-out", str(tmp / "tool.div2.tsv")], tmp)                # E = 0, no ends, no other file
    assert r.returncode == 0, r.stderr[-3000:]
    assert alone.read_bytes() == (dirs["narrow"] / CHAIN).read_bytes()


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and "g.block_lift_joined.tsv" in same and CHAIN not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["narrow"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["narrow"])) - set(same)) == [CHAIN]
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "narrow")}
    assert [s for s in stages["narrow"] if s.startswith("block_chain")] == ["block_chain"] + ["block_chain:" + t for t in ("chain_blocks_scan", "chain_blocks_emit", "chain_text")]
    assert stages["narrow"].index("block_chain") > stages["narrow"].index("block_paf")
    assert [s for s in stages["narrow"] if not s.startswith("block_chain")] == stages["without"]

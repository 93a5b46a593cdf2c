"""`ntSynt --block-maf-multi` and `bin/ntsynt_block_stats --multi-maf-out` end to end (ntsynt_amd/assess.py block_multi_mafs;
docs/design/04_30_block_maf_multi.md) on the family of tests/test_gpu_block_paf.py -- three genomes of 120 kbp with the planted indels --
with --identity-max-edits 1023 --block-ends, and again with E = 0 and no ends.  The expected file is recomputed without the GPU: the
pairwise `--block-maf` rows of the star pairs (the PAF names their blocks) are trimmed to their cores and read back as CIGARs, and
tests/multi_maf_brute.py pads them, makes the rows and lays the sub-blocks out.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import pytest

from ntsynt_amd import assess
from tests import extend_brute as X
from tests import maf_brute as MB
from tests import multi_maf_brute as MM
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, ROOT, SWITCHES, _run, paf_family, read_fasta, records_of

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
PAF, MAF, MULTI = "g.block_alignments.paf", "g.block_alignments.maf", "g.block_alignments.multi.maf"
WIDE = ["--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
TIMERS = ["cigar_pad_sites", "cigar_pad_emit", "cigar_rows_scan", "cigar_rows_emit"]


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 1023 with ends without the switch and with it; E = 0 without ends with it"
    tmp = tmp_path_factory.mktemp("multi_maf_runs")
    paths, _ = paf_family(str(tmp))
    dirs = {}
    for key, switches in (("without", SWITCHES + ["--block-paf", "--block-maf"]), ("full", SWITCHES + ["--block-paf", "--block-maf", "--block-maf-multi"]),
                          ("narrow", ["--block-paf", "--block-maf", "--block-maf-multi"]), ("alone", ["--block-maf-multi"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def star_chains(run_dir):
    """per block, in file order: (reference name, reference length, chains, sites) for tests/multi_maf_brute.table, from the run's PAF
    and pairwise MAF alone: the star pairs' rows trimmed to their cores"""
    table = assess.read_blocks(str(run_dir / "g.synteny_blocks.tsv"))
    lines_of = {table[lines[0]].block_id: [table[i] for i in lines] for _, lines in assess._block_order(table)}
    records = records_of((run_dir / PAF).read_text())
    blocks = MB.parse_maf((run_dir / MAF).read_text())
    assert len(records) == len(blocks)
    groups = {}
    for r, b in zip(records, blocks):
        lines = lines_of[type(next(iter(lines_of)))(r["block"])]
        if r["tg"] != lines[0].genome:
            continue                                          # (no star pair)
        row = [ln.genome for ln in lines].index(r["qg"])
        both = [i for i, (a, q) in enumerate(zip(b["t_row"], b["q_row"])) if a != "-" and q != "-"]
        if not both:
            continue
        lo, hi = both[0], both[-1] + 1
        row_a, row_b = b["t_row"][lo:hi], b["q_row"][lo:hi]
        entries = []
        for a, q in zip(row_a, row_b):
            code = MM.I if a == "-" else MM.D if q == "-" else MM.EQ
            if entries and entries[-1] & 15 == code:
                entries[-1] += 16
            else:
                entries.append(16 | code)
        t0 = b["t_start"] + lo - b["t_row"][:lo].count("-")
        start = b["q_start"] + lo - b["q_row"][:lo].count("-")
        groups.setdefault(r["block"], (b["t_name"], b["t_src_size"], []))[2].append(
            dict(row=row, t0=t0, t1=t0 + MM.len_a(entries), name=b["q_name"], src_size=b["q_src_size"], minus=b["q_strand"] == "-", start=start,
                 entries=entries, a=row_a.replace("-", ""), b=row_b.replace("-", "")))
    out = []
    for block_id in lines_of:
        if str(block_id) not in groups:
            continue
        name, size, chains = groups[str(block_id)]
        chains.sort(key=lambda c: (c["row"], c["t0"]))
        sites = MM.widths([(0, c["t0"], c["entries"]) for c in chains]).get(0, {})
        for c in chains:
            c["row_a"], c["row_b"] = MM.padded_rows(MM.pad_chain(c["entries"], c["t0"], sites), c["a"], c["b"])
        out.append((name, size, chains, sites))
    return out


def test_the_file_equals_the_brute_force_table(runs):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        groups = star_chains(dirs[key])
        assert len(groups) >= 2 and any(g[3] for g in groups)
        got, want = (dirs[key] / MULTI).read_text(), MM.table(groups)
        assert got.count("\n") == want.count("\n")
        assert got == want, [(g[:150], w[:150]) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:2]
    assert (dirs["alone"] / MULTI).read_bytes() == (dirs["narrow"] / MULTI).read_bytes() and not (dirs["alone"] / PAF).exists()
    assert (dirs["narrow"] / MULTI).read_bytes() != (dirs["full"] / MULTI).read_bytes()


def test_rows_hold_the_fasta_bases_and_sub_blocks_do_not_overlap(runs):
    _, paths, dirs = runs
    genomes = {os.path.basename(p): read_fasta(p) for p in paths}
    for key in ("full", "narrow"):
        blocks = MM.parse((dirs[key] / MULTI).read_text())
        assert len(blocks) >= 3 and max(len(b) for b in blocks) == 3 and {r[3] for b in blocks for r in b} == {"+", "-"}
        padded = 0
        for group in star_chains(dirs[key]):                  # (the file is these groups' sub-blocks one behind the other: the test above)
            end = 0
            for sub in MM.parse(MM.MAF_HEADER + MM.group_blocks(*group)):
                assert sub[0][1] >= end, "the sub-blocks of one block ascend and do not overlap on the reference"
                end = sub[0][1] + sub[0][2]
        for b in blocks:
            assert len(b) >= 2 and len({len(r[5]) for r in b}) == 1
            for name, start, size, strand, src, row in b:
                genome, contig = name.split(".fa.")
                seq = genomes[genome + ".fa"][contig]
                assert src == seq.size
                at = src - start - size if strand == "-" else start                                            # back from the reverse strand
                mine = seq[at:at + size]
                assert row.replace("-", "") == MB.letters(X.revcomp(mine) if strand == "-" else mine), (name, start, size, strand)
            for col in range(len(b[0][5])):                   # a P: the reference has a gap, a row has a base and another row a gap
                if b[0][5][col] == "-" and len(b) == 3 and {b[1][5][col], b[2][5][col]} & {"-"} and {b[1][5][col], b[2][5][col]} - {"-"}:
                    padded += 1
        print(key, len(blocks), "sub-blocks,", sum(len(b[0][5]) for b in blocks), "columns,", padded, "padding columns beside a base")
        assert padded > 0, "the family has no site with a P in a row"


def test_the_projection_on_a_star_pair_is_the_core_of_its_pairwise_rows(runs):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        want = {}
        for name, _, chains, _ in star_chains(dirs[key]):
            for c in chains:
                want.setdefault((name, c["name"]), []).append((c["t0"], MM.padded_rows([v for v in c["entries"]], c["a"], c["b"])))
        got = {}
        for b in MM.parse((dirs[key] / MULTI).read_text()):
            for r in b[1:]:
                cols = [(a, q) for a, q in zip(b[0][5], r[5]) if (a, q) != ("-", "-")]
                mine = got.setdefault((b[0][0], r[0]), ["", ""])
                mine[0] += "".join(a for a, _ in cols)
                mine[1] += "".join(q for _, q in cols)
        assert sorted(got) == sorted(want)
        for pair, chains in want.items():
            assert got[pair][0] == "".join(rows[0] for _, rows in chains) and got[pair][1] == "".join(rows[1] for _, rows in chains), pair


def test_the_planted_deletion_is_40_gap_bytes_in_its_row_and_bases_in_the_others(runs):
    _, _, dirs = runs
    gaps = {"fam1.fa.chr1": 0, "fam2.fa.chr1": 0}
    held = dict(gaps)
    for b in MM.parse((dirs["full"] / MULTI).read_text()):
        if b[0][0] != "fam0.fa.chr1":
            continue
        at = b[0][1]
        for col, a in enumerate(b[0][5]):
            if a != "-" and 49_800 <= at < 50_300:
                for r in b[1:]:
                    gaps[r[0]] += r[5][col] == "-"
                    held[r[0]] += r[5][col] != "-"
            at += a != "-"
    assert gaps == {"fam1.fa.chr1": 0, "fam2.fa.chr1": 40} and held == {"fam1.fa.chr1": 500, "fam2.fa.chr1": 460}, (gaps, held)


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and MAF in same and MULTI not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == [MULTI]
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "full")}
    assert [s for s in stages["full"] if s.startswith("block_maf_multi")] == ["block_maf_multi"] + ["block_maf_multi:" + t for t in TIMERS]
    assert stages["full"].index("block_maf_multi") > stages["full"].index("block_maf")
    assert [s for s in stages["full"] if not s.startswith("block_maf_multi")] == stages["without"]


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    out, alone = tmp / "tool.multi.maf", tmp / "tool_alone.multi.maf"
    r = _run(tool + ["--multi-maf-out", str(out), "--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.ends.tsv"), "--ends-max-len",
                     str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_bytes() == (dirs["full"] / MULTI).read_bytes()
    r = _run(tool + ["--multi-maf-out", str(alone), "--divergence-out", str(tmp / "tool.div2.tsv")], tmp)           # E = 0, no ends
    assert r.returncode == 0, r.stderr[-3000:]
    assert alone.read_bytes() == (dirs["narrow"] / MULTI).read_bytes()


def test_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _ = runs
    r = _run(NTSYNT + paths + PARAMS + WIDE + ["--block-maf-multi", "--dry-run"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    listed = [ln for ln in (r.stdout + r.stderr).splitlines() if "block_maf_multi (" in ln]
    assert len(listed) == 1 and "block_maf_multi (" + ", ".join(TIMERS) + "; k " in listed[0] and f"max_edits {MAX_EDITS}" in listed[0] and \
        f"ends_max_len {ENDS_MAX_LEN}" in listed[0], listed
    r = _run(NTSYNT + paths + PARAMS + ["--block-maf-multi"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "--block-maf-multi works from the genomes resident on one GPU" in r.stderr and "--multi-maf-out" in r.stderr, r.stderr[-2000:]

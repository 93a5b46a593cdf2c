"""`ntSynt --block-conservation` and `bin/ntsynt_block_stats --conservation-out --conservation-stats-out` end to end
(ntsynt_amd/assess.py block_conservation; docs/design/04_31_block_conservation.md) on the family of tests/test_gpu_block_paf.py -- three
genomes of 120 kbp with the planted indels -- with --identity-max-edits 1023 --block-ends, and again with E = 0 and no ends.  Both
files are recomputed without the GPU from the run's PAF alone: the cg:Z: CIGARs of the star pairs' records are trimmed to their cores
and tests/conservation_brute.py counts them base by base.  Every test runs under a time limit of its own."""
import faulthandler
import os
import re
import sys

import pytest

from ntsynt_amd import assess
from tests import conservation_brute as CB
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import BAND, ENDS_MAX_EDITS, ENDS_MAX_LEN, ENDS_PENALTY, K, MAX_EDITS, MAX_LEN, RATE, ROOT, SWITCHES, _run, paf_family, records_of

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
PAF, BED, TSV = "g.block_alignments.paf", "g.block_conservation.bed", "g.block_conservation.tsv"
WIDE = ["--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
TIMERS = ["cigar_depth_events", "cigar_depth_emit"]
CODES = {"I": CB.I, "D": CB.D, "=": CB.EQ, "X": CB.X}
PARAMETERS = {"full": (K, RATE, BAND, MAX_LEN, MAX_EDITS, (ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY)), "narrow": (K, RATE, BAND, MAX_LEN, 0, None)}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 1023 with ends without the switch and with it; E = 0 without ends with it"
    tmp = tmp_path_factory.mktemp("conservation_runs")
    paths, _ = paf_family(str(tmp))
    dirs = {}
    for key, switches in (("without", SWITCHES + ["--block-paf"]), ("full", SWITCHES + ["--block-paf", "--block-conservation"]),
                          ("narrow", ["--block-paf", "--block-conservation"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def star_cores(run_dir):
    "(groups, chains) for tests/conservation_brute.py from the run's block table and PAF alone: the star pairs' CIGARs trimmed to their cores"
    table = assess.read_blocks(str(run_dir / "g.synteny_blocks.tsv"))
    lines_of = {}
    for r in table:
        lines_of.setdefault(r.block_id, []).append(r)
    order = sorted(lines_of, key=lambda b: (0, int(b), "") if b.lstrip("-").isdigit() else (1, 0, b))
    groups = [(b, lines_of[b][0].genome, lines_of[b][0].contig, lines_of[b][0].start, lines_of[b][0].end, len(lines_of[b]) - 1) for b in order]
    chains = []
    for r in records_of((run_dir / PAF).read_text()):
        lines = lines_of[r["block"]]
        if r["tg"] != lines[0].genome:
            continue                                          # (no star pair)
        entries = [int(n) << 4 | CODES[c] for n, c in re.findall(r"(\d+)([ID=X])", r["cg"])]
        assert "".join(f"{v >> 4}{'?ID????=X'[v & 15]}" for v in entries) == r["cg"]
        both = [i for i, v in enumerate(entries) if v & 15 in (CB.EQ, CB.X)]
        if not both:
            continue
        t0 = r["t_from"] + sum(v >> 4 for v in entries[:both[0]] if v & 15 == CB.D)
        chains.append((order.index(r["block"]), t0, entries[both[0]:both[-1] + 1]))
    chains.sort(key=lambda c: c[0])
    return groups, chains


def test_both_files_equal_the_brute_force_texts(runs):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        groups, chains = star_cores(dirs[key])
        segs, _ = CB.segments(chains, len(groups))
        assert len(groups) >= 2 and max(g[5] for g in groups) == 2 and {s[3] for s in segs} == {1, 2} and any(s[5] for s in segs)
        assert any(s[3] - s[4] - s[5] for s in segs), "the family has mismatches"
        for name, want in ((BED, CB.bed_text(groups, segs, PARAMETERS[key])), (TSV, CB.table_text(groups, segs, PARAMETERS[key]))):
            got = (dirs[key] / name).read_text()
            assert got.count("\n") == want.count("\n"), (key, name, got.count("\n"), want.count("\n"))
            assert got == want, (key, name, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:2])
    assert (dirs["narrow"] / BED).read_bytes() != (dirs["full"] / BED).read_bytes()


def test_the_table_is_integers_and_its_histograms_add_up(runs):
    _, _, dirs = runs
    lines = (dirs["full"] / TSV).read_text().splitlines()
    assert lines[0].split("\t") == list(assess.CONSERVATION_COLUMNS) and lines[-1].startswith("# k ")
    assert len(lines) > 3
    most = 0
    for line in lines[1:-1]:
        f = line.split("\t")
        rows, covered, core, conserved = (int(v) for v in f[5:9])
        assert rows >= 1
        by_aligned, by_match = [int(v) for v in f[9].split(",")], [int(v) for v in f[10].split(",")]
        assert len(by_aligned) == rows and len(by_match) == rows + 1
        assert sum(by_aligned) == covered and by_aligned[-1] == core == sum(by_match) and by_match[-1] == conserved
        assert 0 <= conserved <= core <= covered <= int(f[4]) - int(f[3]) + 2 * ENDS_MAX_LEN, line
        assert "." not in line.split("\t", 3)[3], "integers only: no ratio is printed"
        most = max(most, conserved)
    assert most > 1000


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and BED not in same and TSV not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == [BED, TSV]
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "full")}
    assert [s for s in stages["full"] if s.startswith("block_conservation")] == ["block_conservation"] + ["block_conservation:" + t for t in TIMERS]
    assert stages["full"].index("block_conservation") > stages["full"].index("block_paf")
    assert [s for s in stages["full"] if not s.startswith("block_conservation")] == stages["without"]
    assert not any("cigar_depth" in s for s in stages["without"])


def test_the_tool_reproduces_both_files(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    r = _run(tool + ["--conservation-out", str(tmp / "tool.bed"), "--conservation-stats-out", str(tmp / "tool.tsv"), "--identity-max-edits", str(MAX_EDITS),
                     "--ends-out", str(tmp / "tool.ends.tsv"), "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.bed").read_bytes() == (dirs["full"] / BED).read_bytes() and (tmp / "tool.tsv").read_bytes() == (dirs["full"] / TSV).read_bytes()
    r = _run(tool + ["--conservation-out", str(tmp / "alone.bed"), "--conservation-stats-out", str(tmp / "alone.tsv"), "--divergence-out",
                     str(tmp / "tool.div2.tsv")], tmp)        # E = 0, no ends
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.bed").read_bytes() == (dirs["narrow"] / BED).read_bytes() and (tmp / "alone.tsv").read_bytes() == (dirs["narrow"] / TSV).read_bytes()
    r = _run(tool + ["--conservation-out", str(tmp / "lonely.bed")], tmp)
    assert r.returncode == 2 and "--conservation-out and --conservation-stats-out go together" in r.stderr


def test_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _ = runs
    r = _run(NTSYNT + paths + PARAMS + WIDE + ["--block-conservation", "--dry-run"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    listed = [ln for ln in (r.stdout + r.stderr).splitlines() if "block_conservation (" in ln]
    assert len(listed) == 1 and "block_conservation (" + ", ".join(TIMERS) + "; k " in listed[0] and f"max_edits {MAX_EDITS}" in listed[0] and \
        f"ends_max_len {ENDS_MAX_LEN}" in listed[0], listed
    r = _run(NTSYNT + paths + PARAMS + ["--block-conservation"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "--block-conservation works from the genomes resident on one GPU" in r.stderr and "--conservation-out" in r.stderr, \
        r.stderr[-2000:]

"""`ntSynt --block-consensus` and `bin/ntsynt_block_stats --profile-out --consensus-out` end to end (ntsynt_amd/assess.py
block_consensus; docs/design/04_33_block_consensus.md) on the family of tests/test_gpu_block_paf.py -- three genomes of 120 kbp with the
planted indels -- with --identity-max-edits 1023 --block-ends, and again with E = 0 and no ends, each run with --block-paf --paf-cs
--block-conservation --block-consensus.  Both files are recomputed without the GPU from the run's PAF alone: the star cores from the
cg:Z: CIGARs and cs:Z: texts as tests/test_gpu_block_variant_sites.py makes them, the reference records from the input FASTA by a plain
parser, and tests/profile_brute.py walks them column by column.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import pytest

from ntsynt_amd import assess
from tests import profile_brute as PB
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import BAND, ENDS_MAX_EDITS, ENDS_MAX_LEN, ENDS_PENALTY, K, MAX_EDITS, MAX_LEN, RATE, ROOT, SWITCHES, _run, paf_family
from tests.test_gpu_block_variant_sites import star_cores

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
PAF, BED, PROFILE, FASTA = "g.block_alignments.paf", "g.block_conservation.bed", "g.block_profile.tsv", "g.block_consensus.fa"
WIDE = ["--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
OTHERS = ["--block-paf", "--paf-cs", "--block-conservation"]
TIMERS = ["cigar_var_bases_scan", "cigar_var_bases_emit", "cigar_profile_events", "cigar_profile_emit"]
PARAMETERS = {"full": (K, RATE, BAND, MAX_LEN, MAX_EDITS, (ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY)), "narrow": (K, RATE, BAND, MAX_LEN, 0, None)}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 1023 with ends without the switch and with it; E = 0 without ends with it"
    tmp = tmp_path_factory.mktemp("consensus_runs")
    paths, _ = paf_family(str(tmp))
    dirs = {}
    for key, switches in (("without", SWITCHES + OTHERS), ("full", SWITCHES + OTHERS + ["--block-consensus"]), ("narrow", OTHERS + ["--block-consensus"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def records_of(path):
    "a plain FASTA parser: {record name: its letters in upper case, what is no base as N}"
    out, name = {}, None
    with open(path, encoding="utf-8") as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                out[name] = []
            elif line.strip():
                out[name].append(line.strip().upper())
    return {k: "".join(ch if ch in "ACGT" else "N" for ch in "".join(v)) for k, v in out.items()}


@pytest.fixture(scope="module")
def brute(runs):
    "per run: (the brute force's columns, the table's text, the FASTA's text), from the run's PAF and the input FASTA alone"
    _, paths, dirs = runs
    genomes = {os.path.basename(p): records_of(p) for p in paths}
    out = {}
    for key in ("full", "narrow"):
        groups, chains, _, alts, ref, _ = star_cores(dirs[key])
        refs, at = [], 0
        for _, _, entries in chains:
            n = PB.byte_counts(entries)[0]
            refs.append(ref[at:at + n])
            at += n
        assert at == len(ref)
        cols, _ = PB.columns(chains, refs, alts, len(groups))
        extents = PB.extents(chains, len(groups))
        bases = [genomes[g[1]][g[2]][e[0]:e[1]] if e is not None else None for g, e in zip(groups, extents)]
        out[key] = (cols, PB.table_text(groups, cols, PARAMETERS[key]), PB.fasta_text(groups, cols, extents, bases))
    return out


def test_both_files_equal_the_brute_force_texts(runs, brute):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        cols, table, fasta = brute[key]
        changed = sum(1 for c in cols if c[8] != c[7])
        print(key, sum(1 for c in cols if c[2] == PB.REF), "reference columns;", sum(1 for c in cols if c[2] != PB.REF), "insertion columns;", changed, "changed calls")
        assert len(cols) > 100 and any(c[2] != PB.REF for c in cols) and changed >= 1
        got = (dirs[key] / PROFILE).read_text()
        assert got.count("\n") == table.count("\n"), (key, got.count("\n"), table.count("\n"))
        assert got == table, (key, [(g, w) for g, w in zip(got.splitlines(), table.splitlines()) if g != w][:2])
        got = (dirs[key] / FASTA).read_text()
        assert [ln for ln in got.splitlines() if ln.startswith(">")] == [ln for ln in fasta.splitlines() if ln.startswith(">")], key
        assert got == fasta, key
        assert any(int(ln.split("changed=")[1]) >= 1 for ln in got.splitlines() if ln.startswith(">")), "a block whose consensus differs from its reference"
    assert (dirs["narrow"] / PROFILE).read_bytes() != (dirs["full"] / PROFILE).read_bytes()


def test_the_reference_columns_sum_to_the_conservation_bed(runs, brute):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        lines = (dirs[key] / PROFILE).read_text().splitlines()
        assert lines[0].split("\t") == list(assess.PROFILE_COLUMNS) and lines[-1].startswith("# k ")
        rows = [ln.split("\t") for ln in lines[1:-1]]
        bed = [ln.split("\t") for ln in (dirs[key] / BED).read_text().splitlines() if not ln.startswith("#")]
        mismatches = sum((int(f[6]) - int(f[7]) - int(f[9])) * (int(f[2]) - int(f[1])) for f in bed)
        gaps = sum(int(f[9]) * (int(f[2]) - int(f[1])) for f in bed)
        ours = [c for c in brute[key][0] if c[2] == PB.REF]    # (the columns behind the file: test_both_files_equal_the_brute_force_texts)
        assert len(ours) == sum(1 for f in rows if f[2] == ".")
        assert sum(c[3] - c[4] - c[5] for c in ours) == mismatches > 100, key
        assert sum(c[5] for c in ours) == gaps == sum(int(f[13]) for f in rows if f[2] == "."), key
        for f in rows:
            assert sum(int(x) for x in f[8:14]) == int(f[6]) <= int(f[5]) + 1 and f[7] in "ACGTN-" and f[14] in "ACGTN-" and (f[7] == "-") == (f[2] != "."), f


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and BED in same and PROFILE not in same and FASTA not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == sorted([PROFILE, FASTA])
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "full")}
    assert [s for s in stages["full"] if s.startswith("block_consensus")] == ["block_consensus"] + ["block_consensus:" + t for t in TIMERS]
    assert stages["full"].index("block_consensus") > stages["full"].index("block_conservation")
    assert [s for s in stages["full"] if not s.startswith("block_consensus")] == stages["without"]
    assert not any("cigar_var_bases" in s or "cigar_profile" in s for s in stages["without"])


def test_the_tool_reproduces_both_files(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    r = _run(tool + ["--profile-out", str(tmp / "tool.profile.tsv"), "--consensus-out", str(tmp / "tool.consensus.fa"), "--identity-max-edits", str(MAX_EDITS),
                     "--ends-out", str(tmp / "tool.ends.tsv"), "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.profile.tsv").read_bytes() == (dirs["full"] / PROFILE).read_bytes()
    assert (tmp / "tool.consensus.fa").read_bytes() == (dirs["full"] / FASTA).read_bytes()
    r = _run(tool + ["--profile-out", str(tmp / "alone.profile.tsv"), "--consensus-out", str(tmp / "alone.consensus.fa"),
                     "--divergence-out", str(tmp / "tool.div2.tsv")], tmp)        # E = 0, no ends
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.profile.tsv").read_bytes() == (dirs["narrow"] / PROFILE).read_bytes()
    assert (tmp / "alone.consensus.fa").read_bytes() == (dirs["narrow"] / FASTA).read_bytes()
    r = _run(tool + ["--profile-out", str(tmp / "half.profile.tsv")], tmp)
    assert r.returncode == 2 and "--profile-out and --consensus-out go together" in r.stderr, r.stderr[-2000:]


def test_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _ = runs
    r = _run(NTSYNT + paths + PARAMS + WIDE + ["--block-consensus", "--dry-run"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    listed = [ln for ln in (r.stdout + r.stderr).splitlines() if "block_consensus (" in ln]
    assert len(listed) == 1 and "block_consensus (" + ", ".join(TIMERS) + "; k " in listed[0] and f"max_edits {MAX_EDITS}" in listed[0] and \
        f"ends_max_len {ENDS_MAX_LEN}" in listed[0], listed
    r = _run(NTSYNT + paths + PARAMS + ["--block-consensus"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "--block-consensus works from the genomes resident on one GPU" in r.stderr and "--profile-out" in r.stderr, \
        r.stderr[-2000:]

"""`ntSynt --block-lift BED --lift-genome NAME` and `bin/ntsynt_block_stats --lift-bed --lift-genome --lift-out` end to end
(ntsynt_amd/assess.py block_lift; docs/design/04_23_block_lift.md) on the family and with the parameters of tests/test_gpu_block_paf.py.
Runs: --block-paf ... --block-ends --identity-max-edits 1023 without the lift; the same with the lift of fam1.fa (line a against fam2.fa,
line b against fam0.fa); with the lift of fam2.fa (always line b; its second record is `-`); and the lift of fam0.fa alone, without
--block-paf.  The BED files hold, per contig, intervals well inside blocks, genome 0's bases 50 010 .. 50 030 of chr1 (inside the planted
40-base deletion of genome 2), intervals across an inversion border, across chain ends, in the unrelated tail, over the run of N, the
whole contig, and, taken from the first run's PAF, 1-base intervals at chains' first and last bases and an interval inside the longest gap run.  Each lift file's body equals
tests/lift_brute.lift_from_paf of the same run's PAF; lifted end points that lie in `=` columns carry the same base in both FASTA files;
the tool reproduces the file; every other file is that of the run without the switch.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import pytest

from ntsynt_amd import assess
from tests import lift_brute as LB
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, PARAMS, STEP_SECONDS, SWITCHES, paf_family, read_fasta, records_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
COMPLEMENT = {ord(a): ord(b) for a, b in zip("ACGT", "TGCA")}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _run(cmd, cwd, **env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT, **env))


def bed_of(source, sizes, records):
    "the BED lines of one source genome: sizes = {contig: bases}, records = the first run's PAF records"
    out = [("chr1", 5_000, 5_100, "inside"), ("chr1", 40_000, 40_250, "inside"), ("chr2", 10_000, 10_100, "inside"), ("chr1", 50_010, 50_030, "deleted_in_2"),
           ("chr1", 23_950, 24_050, "inversion_border"), ("chr2", 27_950, 28_050, "inversion_border"), ("chr2", 1_000, 1_100, "tail_of_2"),
           ("chr2", 57_000, 57_100, "tail"), ("chr2", 55_950, 56_350, "run_of_N")] + [(c, 0, n, "whole") for c, n in sorted(sizes.items())]
    as_target = [r for r in records if r["tg"] == source][:5]
    as_query = [r for r in records if r["qg"] == source][:5]
    for r in as_target:
        out += [(r["t"], r["t_from"], r["t_from"] + 1, "first_base"), (r["t"], r["t_to"] - 1, r["t_to"], "last_base"),
                (r["t"], max(r["t_to"] - 20, 0), min(r["t_to"] + 20, sizes[r["t"]]), "chain_end")]
    for r in as_query:
        out += [(r["q"], r["q_from"], r["q_from"] + 1, "first_base"), (r["q"], r["q_to"] - 1, r["q_to"], "last_base"),
                (r["q"], max(r["q_from"] - 20, 0), min(r["q_from"] + 20, sizes[r["q"]]), "chain_end")]
    gap = None                                                # the longest run of the source's bases that the other genome lacks, but for its rim
    for r in records:
        if source not in (r["tg"], r["qg"]):
            continue
        walker = LB.Walker(LB.parse_cigar(r["cg"]))
        i = j = 0
        for v in LB.parse_cigar(r["cg"]):
            length, code = v >> 4, v & 15
            if code == (2 if r["tg"] == source else 1) and length >= 6 and (gap is None or length > gap[2] - gap[1] + 2):
                at = r["t_from"] + i if r["tg"] == source else (r["q_to"] - j - length if r["sign"] == "-" else r["q_from"] + j)
                gap = (r["t"] if r["tg"] == source else r["q"], at + 1, at + length - 1, "in_a_gap")
            i, j = i + (length if code != 1 else 0), j + (length if code != 2 else 0)
        assert (i, j) == (walker.len_a, walker.len_b)
    assert (as_target or as_query) and gap is not None
    out.append(gap)
    return [b for b in out if b[1] < b[2] <= sizes[b[0]]]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lift_runs")
    paths, fam = paf_family(str(tmp))
    names = [os.path.basename(p) for p in paths]
    sizes = {name: {f"chr{i + 1}": int(c.size) for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    full = SWITCHES + ["--block-paf"]
    dirs = {"without": tmp / "without"}
    dirs["without"].mkdir()
    r = _run(NTSYNT + paths + PARAMS + full, dirs["without"])
    assert r.returncode == 0, r.stderr[-3000:]
    records = records_of((dirs["without"] / "g.block_alignments.paf").read_text())
    beds = {}
    for name in names:
        beds[name] = bed_of(name, sizes[name], records)
        (tmp / f"{name}.bed").write_text("# intervals of " + name + "\n" + "".join("\t".join(str(v) for v in b) + "\n" for b in beds[name]))
    for name, switches in (("fam1.fa", full), ("fam2.fa", full), ("fam0.fa", [s for s in SWITCHES if s != "--block-identity"])):
        dirs[name] = tmp / name.replace(".", "_")
        dirs[name].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches + ["--block-lift", str(tmp / f"{name}.bed"), "--lift-genome", name], dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs, beds


def body_of(text):
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.LIFT_COLUMNS) and lines[-1].startswith("# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500")
    return lines[1:-1]


def test_each_file_equals_the_walk_over_the_same_runs_paf(runs):
    tmp, _, dirs, beds = runs
    for name in ("fam1.fa", "fam2.fa", "fam0.fa"):
        paf = (dirs[name if name != "fam0.fa" else "without"] / "g.block_alignments.paf").read_text()      # (fam0.fa: lifted without --block-paf)
        want, _ = LB.lift_from_paf(paf, beds[name], name)
        got = body_of((dirs[name] / "g.block_lift.tsv").read_text())
        print(name, len(beds[name]), "intervals,", len(got), "lines")
        assert len(got) == len(want) >= len(beds[name])
        assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:2]
    assert not (dirs["fam0.fa"] / "g.block_alignments.paf").exists()                        # (the switch works alone)


def rows_of(path):
    return [dict(zip(assess.LIFT_COLUMNS, ln.split("\t"))) for ln in body_of(path.read_text())]


def test_the_cases_the_bed_files_were_made_for_occur(runs):
    _, _, dirs, _ = runs
    one, two, zero = (rows_of(dirs[n] / "g.block_lift.tsv") for n in ("fam1.fa", "fam2.fa", "fam0.fa"))
    for rows in (one, two, zero):
        assert any(r["status"] == "unmapped" for r in rows) and any(r["status"] == "partial" for r in rows) and any(r["status"] == "full" for r in rows)
        assert any(r["orientation"] == "-" for r in rows)
    # fam1.fa is line a against fam2.fa and line b against fam0.fa; fam2.fa is line b of every pair
    assert {r["to_genome"] for r in one if r["status"] != "unmapped"} == {"fam0.fa", "fam2.fa"}
    assert {r["to_genome"] for r in two if r["status"] != "unmapped"} == {"fam0.fa", "fam1.fa"}
    # genome 0's bases 50 010 .. 50 030 lie inside the 40 bases that were cut out of genome 2: genome 1 has all 20 of them; in genome 2 the
    # canonical script of the stretch splits the deletion around bases that match by chance (..TCGCAAC.. against the TGCAAC behind it), so
    # fewer than 20 are left but not none; the interval taken from the longest gap run of the PAF itself lifts to length 0
    gone = {r["to_genome"]: r for r in zero if r["name"] == "deleted_in_2"}
    assert sorted(gone) == ["fam1.fa", "fam2.fa"] and int(gone["fam1.fa"]["to_end"]) - int(gone["fam1.fa"]["to_start"]) == 20
    assert 0 <= int(gone["fam2.fa"]["to_end"]) - int(gone["fam2.fa"]["to_start"]) < 20
    assert all(r["status"] == "full" and (r["src_start"], r["src_end"]) == ("50010", "50030") for r in gone.values())
    for rows in (one, two, zero):
        inside = [r for r in rows if r["name"] == "in_a_gap" and r["to_start"] == r["to_end"]]
        assert inside and all(r["status"] == "full" and int(r["src_start"]) < int(r["src_end"]) for r in inside), [r for r in rows if r["name"] == "in_a_gap"]
    whole = [r for r in one if r["name"] == "whole" and r["contig"] == "chr1"]
    assert len(whole) >= 3 and all(r["status"] == "partial" for r in whole)                 # an interval over several chains: a line per chain


def test_lifted_end_points_in_equal_columns_carry_the_same_base(runs):
    _, paths, dirs, beds = runs
    genomes = {os.path.basename(p): read_fasta(p) for p in paths}
    checked = {"+": 0, "-": 0}
    for name in ("fam1.fa", "fam2.fa"):
        _, in_equal = LB.lift_from_paf((dirs[name] / "g.block_alignments.paf").read_text(), beds[name], name)
        rows = rows_of(dirs[name] / "g.block_lift.tsv")
        assert len(rows) == len(in_equal)
        for r, equal in zip(rows, in_equal):
            if r["status"] != "full" or not equal:
                continue
            src, oth = genomes[name][r["contig"]], genomes[r["to_genome"]][r["to_contig"]]
            start, end, to_start, to_end = (int(r[f]) for f in ("start", "end", "to_start", "to_end"))
            if r["orientation"] == "+":
                assert (src[start], src[end - 1]) == (oth[to_start], oth[to_end - 1]), r
            else:
                assert (src[start], src[end - 1]) == (COMPLEMENT[int(oth[to_end - 1])], COMPLEMENT[int(oth[to_start])]), r
            checked[r["orientation"]] += 1
    assert checked["+"] >= 5 and checked["-"] >= 2, checked


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs, _ = runs
    fais = [str(dirs["fam1.fa"] / (os.path.basename(p) + ".fai")) for p in paths]
    common = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["fam1.fa"] / "g.synteny_blocks.tsv"), "--fai"] + fais + \
        ["--fastas"] + paths + ["--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.block_ends.tsv"), "--ends-max-len", str(ENDS_MAX_LEN),
                                "--divergence-out", str(tmp / "tool.div.tsv")]
    for name, extra in (("fam1.fa", []), ("fam2.fa", ["--paf-out", str(tmp / "tool.paf")])):     # the lift alone, and beside the PAF in one pass
        out = tmp / f"tool.{name}.block_lift.tsv"
        r = _run(common + extra + ["--lift-bed", str(tmp / f"{name}.bed"), "--lift-genome", name, "--lift-out", str(out)], tmp)
        assert r.returncode == 0, r.stderr[-3000:]
        assert out.read_bytes() == (dirs[name] / "g.block_lift.tsv").read_bytes()
    assert (tmp / "tool.paf").read_bytes() == (dirs["fam2.fa"] / "g.block_alignments.paf").read_bytes()
    r = _run(common + ["--lift-bed", str(tmp / "fam1.fa.bed"), "--lift-genome", "fam7.fa", "--lift-out", str(tmp / "no.tsv")], tmp)
    assert r.returncode == 2 and "fam7.fa is not among the genomes" in r.stderr
    r = _run(common + ["--lift-bed", str(tmp / "fam1.fa.bed"), "--lift-out", str(tmp / "no.tsv")], tmp)
    assert r.returncode == 2 and "go together" in r.stderr


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs, _ = runs
    same = sorted(os.listdir(dirs["without"]))
    assert "g.block_alignments.paf" in same and "g.block_ends.tsv" in same and not [n for n in same if "block_lift" in n]
    for run in ("fam1.fa", "fam2.fa"):
        for name in same:
            if name != "g.stage_times.tsv":
                assert (dirs["without"] / name).read_bytes() == (dirs[run] / name).read_bytes(), (run, name)
        assert sorted(set(os.listdir(dirs[run])) - set(same)) == ["g.block_lift.tsv"]
        stages = {d: [ln.split("\t")[0] for ln in (dirs[d] / "g.stage_times.tsv").read_text().splitlines()] for d in ("without", run)}
        assert all(s in stages[run] for s in ("block_lift", "block_lift:lift_scan", "block_lift:lift_search"))
        assert [s for s in stages[run] if not s.startswith("block_lift")] == stages["without"]
    alone = [ln.split("\t")[0] for ln in (dirs["fam0.fa"] / "g.stage_times.tsv").read_text().splitlines()]
    assert "block_lift:lift_search" in alone and not [s for s in alone if s.startswith("block_paf")]


def test_an_interval_on_an_unknown_contig_stops_the_run(runs):
    tmp, paths, _, _ = runs
    (tmp / "unknown").mkdir()
    (tmp / "unknown.bed").write_text("chr1\t10\t20\nchr9\t1\t2\n")
    r = _run(NTSYNT + paths + PARAMS + ["--block-lift", str(tmp / "unknown.bed"), "--lift-genome", "fam1.fa"], tmp / "unknown")
    assert r.returncode != 0 and "has no record chr9" in r.stderr


def test_parser_errors_and_the_dry_run(runs):
    tmp, paths, _, _ = runs
    bed = str(tmp / "fam1.fa.bed")
    r = _run(NTSYNT + paths + PARAMS + ["--block-lift", bed], tmp)
    assert r.returncode == 2 and "--lift-genome" in r.stderr
    r = _run(NTSYNT + paths + PARAMS + ["--lift-genome", "fam1.fa"], tmp)
    assert r.returncode == 2 and "--block-lift" in r.stderr
    r = _run(NTSYNT + paths + PARAMS + ["--block-lift", bed, "--lift-genome", "fam9.fa"], tmp)
    assert r.returncode == 2 and "fam9.fa is not among the genomes" in r.stderr
    r = _run(NTSYNT + paths + PARAMS + ["--block-lift", bed, "--lift-genome", "fam1.fa"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "one rank" in r.stderr and "ntsynt_block_stats --tsv" in r.stderr and "--lift-out" in r.stderr
    r = _run(NTSYNT + paths + PARAMS + ["--block-lift", bed, "--lift-genome", "fam1.fa", "--block-paf", "--dry-run"], tmp)
    assert r.returncode == 0 and "block_paf (cigar_atoms, cigar_merge;" in r.stdout and "-> block_lift (lift_scan, lift_search; " in r.stdout, r.stdout
    assert "max_edits 0)" in r.stdout.split("block_lift (")[1]

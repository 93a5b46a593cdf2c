"""`ntSynt --block-lift BED --lift-genome NAME --lift-identity`, `--lift-windows W` and `bin/ntsynt_block_stats --lift-identity-out /
--lift-windows --lift-windows-out` end to end (ntsynt_amd/assess.py block_lift_identity; docs/design/04_25_lift_identity.md) on the family,
the parameters and the BED files of tests/test_gpu_block_lift.py.  Runs: --block-paf ... without the new switches but with the lift of
fam1.fa; the same with --lift-identity and --lift-windows 1000; the lift of fam2.fa with --lift-identity; and fam0.fa with --lift-identity
alone, without --block-paf.  Each file's body equals tests/lift_stats_brute.identity_from_paf of the same run's PAF; its first 14 columns
and its status are block_lift.tsv's; a `whole` interval over an entire chain carries the PAF record's matches; per PAF record the windows'
matches add up to its column 10; the tool reproduces both files; every other file is that of the run without the switches.  Every test
runs under a time limit of its own."""
import faulthandler
import os
import sys

import pytest

from ntsynt_amd import assess
from tests import lift_stats_brute as SB
from tests.test_gpu_block_lift import NTSYNT, ROOT, _run, bed_of
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, PARAMS, STEP_SECONDS, SWITCHES, paf_family, records_of

pytestmark = pytest.mark.gpu
W = 1000


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lift_identity_runs")
    paths, fam = paf_family(str(tmp))
    names = [os.path.basename(p) for p in paths]
    sizes = {name: {f"chr{i + 1}": int(c.size) for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    full = SWITCHES + ["--block-paf"]
    alone = [s for s in SWITCHES if s != "--block-identity"]
    dirs, beds = {}, {}

    def run(key, switches):
        dirs[key] = tmp / ("run_" + key.replace(".", "_"))   # (the FASTA files lie in tmp under the genomes' names)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    # the BED files need a PAF: fam1.fa's comes from a run that is also the yardstick "without the new switches" (it lifts some fixed intervals)
    (tmp / "first.bed").write_text("chr1\t5000\t5100\tinside\n")
    run("without", full + ["--block-lift", str(tmp / "first.bed"), "--lift-genome", "fam1.fa"])
    records = records_of((dirs["without"] / "g.block_alignments.paf").read_text())
    for name in names:
        beds[name] = bed_of(name, sizes[name], records)
        (tmp / f"{name}.bed").write_text("".join("\t".join(str(v) for v in b) + "\n" for b in beds[name]))
    lift = {name: ["--block-lift", str(tmp / f"{name}.bed"), "--lift-genome", name] for name in names}
    run("fam1_lift", full + lift["fam1.fa"])
    run("fam1.fa", full + lift["fam1.fa"] + ["--lift-identity", "--lift-windows", str(W)])
    run("fam2.fa", full + lift["fam2.fa"] + ["--lift-identity"])
    run("fam0.fa", alone + lift["fam0.fa"] + ["--lift-identity"])
    run("windows_alone", alone + ["--lift-genome", "fam1.fa", "--lift-windows", str(W)])
    return tmp, paths, dirs, beds, sizes


def body_of(text):
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.LIFT_IDENTITY_COLUMNS)
    assert lines[-1].startswith("# k 21, rate 16, band 31, max_len 4096, max_edits 1023, ends_max_len 1500")
    return lines[1:-1]


def rows_of(path):
    return [dict(zip(assess.LIFT_IDENTITY_COLUMNS, ln.split("\t"))) for ln in body_of(path.read_text())]


def windows_of(sizes):
    return [(c, s, min(s + W, n), f"w{s // W}") for c, n in sizes.items() for s in range(0, n, W)]


def test_each_file_equals_the_walk_over_the_same_runs_paf(runs):
    _, _, dirs, beds, _ = runs
    for name in ("fam1.fa", "fam2.fa", "fam0.fa"):
        paf = (dirs[name if name != "fam0.fa" else "without"] / "g.block_alignments.paf").read_text()      # (fam0.fa: counted without --block-paf)
        want = SB.identity_from_paf(paf, beds[name], name)
        got = body_of((dirs[name] / "g.block_lift_identity.tsv").read_text())
        print(name, len(beds[name]), "intervals,", len(got), "lines")
        assert len(got) == len(want) >= len(beds[name])
        assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:2]
    assert not (dirs["fam0.fa"] / "g.block_alignments.paf").exists()                        # (the switch works without --block-paf)


def test_the_first_columns_and_the_status_are_the_lift_tables(runs):
    _, _, dirs, _, _ = runs
    for name in ("fam1.fa", "fam2.fa", "fam0.fa"):
        lift = (dirs[name] / "g.block_lift.tsv").read_text().splitlines()[1:-1]
        counted = body_of((dirs[name] / "g.block_lift_identity.tsv").read_text())
        assert len(lift) == len(counted) > 20
        for a, b in zip(lift, counted):
            a, b = a.split("\t"), b.split("\t")
            assert a[:14] == b[:14] and a[14] == b[-1] and len(b) == len(assess.LIFT_IDENTITY_COLUMNS), (a, b)
    statuses = {r["status"] for r in rows_of(dirs["fam1.fa"] / "g.block_lift_identity.tsv")}
    assert statuses == {"full", "partial", "unmapped"}


def test_a_whole_interval_over_an_entire_chain_carries_the_records_matches(runs):
    _, _, dirs, _, _ = runs
    seen = 0
    for name in ("fam1.fa", "fam2.fa"):
        records = records_of((dirs[name] / "g.block_alignments.paf").read_text())
        by_key = {(r["block"], r["tg"] if r["qg"] == name else r["qg"], r["ch"]): r for r in records if name in (r["tg"], r["qg"])}
        for r in rows_of(dirs[name] / "g.block_lift_identity.tsv"):
            if r["name"] != "whole" or r["status"] == "unmapped":
                continue
            rec = by_key[(r["block_id"], r["to_genome"], int(r["ch"]))]
            mine = (rec["t_from"], rec["t_to"]) if rec["tg"] == name else (rec["q_from"], rec["q_to"])
            assert (int(r["src_start"]), int(r["src_end"])) == mine                         # (the whole contig covers the entire chain)
            assert int(r["matches"]) == rec["matches"] and int(r["columns"]) == rec["columns"], (r, rec["matches"], rec["columns"])
            assert int(r["mismatches"]) + int(r["src_gap_bases"]) + int(r["to_gap_bases"]) == rec["nm"]
            seen += 1
    assert seen >= 6


def test_the_windows_equal_the_brute_force_and_add_up_to_each_records_matches(runs):
    _, _, dirs, _, sizes = runs
    paf = (dirs["fam1.fa"] / "g.block_alignments.paf").read_text()
    got = body_of((dirs["fam1.fa"] / "g.block_windows.tsv").read_text())
    want = SB.identity_from_paf(paf, windows_of(sizes["fam1.fa"]), "fam1.fa")
    assert len(got) == len(want) >= sum(-(-n // W) for n in sizes["fam1.fa"].values())
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:2]
    total = {}
    for r in rows_of(dirs["fam1.fa"] / "g.block_windows.tsv"):
        if r["status"] != "unmapped":
            key = (r["block_id"], r["to_genome"], int(r["ch"]))
            total[key] = total.get(key, 0) + int(r["matches"])
    records = [r for r in records_of(paf) if "fam1.fa" in (r["tg"], r["qg"])]
    assert len(records) == len(total) >= 4
    for rec in records:
        assert total[(rec["block"], rec["tg"] if rec["qg"] == "fam1.fa" else rec["qg"], rec["ch"])] == rec["matches"], rec
    # the windows alone, without --block-paf and --block-lift: the same file
    assert (dirs["windows_alone"] / "g.block_windows.tsv").read_bytes() == (dirs["fam1.fa"] / "g.block_windows.tsv").read_bytes()
    assert not [n for n in os.listdir(dirs["windows_alone"]) if "block_lift" in n or n.endswith(".paf")]


def test_the_interval_inside_the_planted_deletion(runs):
    "genome 0's bases 50 010 .. 50 030 of chr1 lie inside the 40 bases cut out of genome 2: bases genome 2 lacks, and no run that genome 0 lacks"
    _, _, dirs, _, _ = runs
    gone = {r["to_genome"]: r for r in rows_of(dirs["fam0.fa"] / "g.block_lift_identity.tsv") if r["name"] == "deleted_in_2"}
    assert sorted(gone) == ["fam1.fa", "fam2.fa"]
    assert int(gone["fam2.fa"]["src_gap_bases"]) > 0 and int(gone["fam2.fa"]["to_gaps"]) == 0 and int(gone["fam2.fa"]["src_gaps"]) >= 1
    assert (gone["fam1.fa"]["src_gap_bases"], gone["fam1.fa"]["to_gap_bases"], gone["fam1.fa"]["columns"]) == ("0", "0", "20")
    for rows in (rows_of(dirs[n] / "g.block_lift_identity.tsv") for n in ("fam1.fa", "fam2.fa", "fam0.fa")):
        inside = [r for r in rows if r["name"] == "in_a_gap" and r["to_start"] == r["to_end"]]
        assert inside and all((r["matches"], r["identity"], r["src_gaps"]) == ("0", "0.000000", "1") for r in inside)


def test_the_tool_reproduces_both_files(runs):
    tmp, paths, dirs, _, _ = runs
    fais = [str(dirs["fam1.fa"] / (os.path.basename(p) + ".fai")) for p in paths]
    common = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["fam1.fa"] / "g.synteny_blocks.tsv"), "--fai"] + fais + \
        ["--fastas"] + paths + ["--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.block_ends.tsv"), "--ends-max-len", str(ENDS_MAX_LEN),
                                "--divergence-out", str(tmp / "tool.div.tsv")]
    # everything in one pass beside the PAF; then the identity alone; then the windows alone
    r = _run(common + ["--paf-out", str(tmp / "tool.paf"), "--lift-bed", str(tmp / "fam1.fa.bed"), "--lift-genome", "fam1.fa", "--lift-out", str(tmp / "tool.lift.tsv"),
                       "--lift-identity-out", str(tmp / "tool.identity.tsv"), "--lift-windows", str(W), "--lift-windows-out", str(tmp / "tool.windows.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.identity.tsv").read_bytes() == (dirs["fam1.fa"] / "g.block_lift_identity.tsv").read_bytes()
    assert (tmp / "tool.windows.tsv").read_bytes() == (dirs["fam1.fa"] / "g.block_windows.tsv").read_bytes()
    assert (tmp / "tool.lift.tsv").read_bytes() == (dirs["fam1.fa"] / "g.block_lift.tsv").read_bytes()
    assert (tmp / "tool.paf").read_bytes() == (dirs["fam1.fa"] / "g.block_alignments.paf").read_bytes()
    r = _run(common + ["--lift-bed", str(tmp / "fam2.fa.bed"), "--lift-genome", "fam2.fa", "--lift-identity-out", str(tmp / "tool.identity2.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.identity2.tsv").read_bytes() == (dirs["fam2.fa"] / "g.block_lift_identity.tsv").read_bytes()
    r = _run(common + ["--lift-genome", "fam1.fa", "--lift-windows", str(W), "--lift-windows-out", str(tmp / "tool.windows1.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.windows1.tsv").read_bytes() == (dirs["fam1.fa"] / "g.block_windows.tsv").read_bytes()
    r = _run(common + ["--lift-genome", "fam1.fa", "--lift-identity-out", str(tmp / "no.tsv")], tmp)
    assert r.returncode == 2 and "--lift-identity-out needs the intervals" in r.stderr


def test_every_other_file_is_that_of_the_run_without_the_switches(runs):
    _, _, dirs, _, _ = runs
    same = sorted(os.listdir(dirs["fam1_lift"]))
    assert "g.block_alignments.paf" in same and "g.block_lift.tsv" in same and not [n for n in same if "lift_identity" in n or "windows" in n]
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["fam1_lift"] / name).read_bytes() == (dirs["fam1.fa"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["fam1.fa"])) - set(same)) == ["g.block_lift_identity.tsv", "g.block_windows.tsv"]
    stages = {d: [ln.split("\t")[0] for ln in (dirs[d] / "g.stage_times.tsv").read_text().splitlines()] for d in ("fam1_lift", "fam1.fa", "windows_alone")}
    new = [s for s in stages["fam1.fa"] if s.startswith(("block_lift_identity", "block_windows"))]
    assert new == [f"{stage}{timer}" for stage in ("block_lift_identity", "block_windows") for timer in ("", ":lift_stats_scan", ":lift_stats_search")]
    assert [s for s in stages["fam1.fa"] if s not in new] == stages["fam1_lift"]
    assert stages["fam1.fa"].index("block_lift_identity") > stages["fam1.fa"].index("block_lift")
    assert "block_windows:lift_stats_search" in stages["windows_alone"] and not [s for s in stages["windows_alone"] if s.startswith(("block_paf", "block_lift"))]
    # the other files of the two runs with other BED files: those of the yardstick run, whose BED differs
    for run in ("fam2.fa", "without"):
        for name in same:
            if name not in ("g.stage_times.tsv", "g.block_lift.tsv"):
                assert (dirs["fam1_lift"] / name).read_bytes() == (dirs[run] / name).read_bytes(), (run, name)

"""`ntSynt --lift-join` with `--block-lift BED` and `--lift-windows W`, and `bin/ntsynt_block_stats --lift-joined-out /
--lift-windows-joined-out`, end to end (ntsynt_amd/assess.py block_lifts; docs/design/04_27_lift_joined.md) on the family of
tests/test_gpu_block_paf.py with E = 0 and without --block-ends, so that the chains break at the large indels.  Each joined file's body
equals tests/lift_pairs_brute.joined_from_paf of the same run's PAF; per (interval, pair) the joined line agrees with that run's
block_lift_identity.tsv lines (their number, the hull of their spans, the sums of their counts, the open bases = hull minus sums); an
interval across the planted 40-base deletion gives ONE line with two chains whose open bases differ by what the PAF leaves unaligned
there; with --identity-max-edits 1023 --block-ends every pair has one chain and the joined counts are the per-chain table's; the tool
reproduces the files; every other file is that of the run without the switch.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import pytest

from ntsynt_amd import assess
from tests import lift_pairs_brute as PB
from tests.test_gpu_block_lift import NTSYNT, ROOT, _run
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, PARAMS, STEP_SECONDS, SWITCHES, paf_family, records_of

pytestmark = pytest.mark.gpu
W = 1000
SOURCE = "fam0.fa"
COUNTS = ("matches", "mismatches", "src_gap_bases", "to_gap_bases", "src_gaps", "to_gaps")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lift_joined_runs")
    paths, fam = paf_family(str(tmp))
    names = [os.path.basename(p) for p in paths]
    sizes = {f"chr{i + 1}": int(c.size) for i, c in enumerate(fam[names.index(SOURCE)])}
    bed = [("chr1", 5_000, 5_100, "inside"), ("chr1", 40_000, 40_250, "inside"), ("chr2", 10_000, 10_100, "inside"), ("chr1", 50_010, 50_030, "deleted_in_2"),
           ("chr1", 49_900, 50_200, "across_deletion"), ("chr1", 44_800, 45_200, "across_insertion"), ("chr1", 23_950, 24_050, "inversion_border"),
           ("chr2", 27_950, 28_050, "inversion_border"), ("chr1", 11_000, 51_000, "long"), ("chr2", 57_000, 57_100, "tail"), ("chr2", 55_950, 56_350, "run_of_N")] + \
        [(c, 0, n, "whole") for c, n in sorted(sizes.items())]
    (tmp / "iv.bed").write_text("".join("\t".join(str(v) for v in b) + "\n" for b in bed))
    lift = ["--block-paf", "--benchmark", "--block-lift", str(tmp / "iv.bed"), "--lift-genome", SOURCE, "--lift-identity", "--lift-windows", str(W)]
    dirs = {}

    def run(key, switches):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    run("without", lift)                                      # E = 0, no ends
    run("joined", lift + ["--lift-join"])
    run("one_chain", [s for s in SWITCHES if s != "--benchmark"] + lift + ["--lift-join"])
    return tmp, paths, dirs, bed, sizes


def rows_of(path, columns):
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(columns) and lines[-1].startswith("# k 21, rate 16, band 31, max_len 4096, max_edits ")
    return lines[1:-1], [dict(zip(columns, ln.split("\t"))) for ln in lines[1:-1]]


def windows_of(sizes):
    return [(c, s, min(s + W, n), f"w{s // W}") for c, n in sizes.items() for s in range(0, n, W)]


def test_each_joined_file_equals_the_walk_over_the_same_runs_paf(runs):
    _, _, dirs, bed, sizes = runs
    for key in ("joined", "one_chain"):
        paf = (dirs[key] / "g.block_alignments.paf").read_text()
        for stem, intervals in (("g.block_lift_joined.tsv", bed), ("g.block_windows_joined.tsv", windows_of(sizes))):
            got, _ = rows_of(dirs[key] / stem, assess.LIFT_JOINED_COLUMNS)
            want = PB.joined_from_paf(paf, intervals, SOURCE)
            print(key, stem, len(intervals), "intervals,", len(got), "lines")
            assert len(got) == len(want) >= len(intervals)
            assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:2]
    chains_per_pair = [len(p) for p in PB.paf_pairs((dirs["joined"] / "g.block_alignments.paf").read_text(), SOURCE)]
    print("chains per pair at E = 0:", chains_per_pair)
    assert max(chains_per_pair) >= 3                          # (the chains break at the large indels)


def test_the_joined_lines_agree_with_the_per_chain_table(runs):
    _, _, dirs, _, _ = runs
    for joined_file, chain_file in (("g.block_lift_joined.tsv", "g.block_lift_identity.tsv"), ("g.block_windows_joined.tsv", "g.block_windows.tsv")):
        _, joined = rows_of(dirs["joined"] / joined_file, assess.LIFT_JOINED_COLUMNS)
        _, chains = rows_of(dirs["joined"] / chain_file, assess.LIFT_IDENTITY_COLUMNS)
        per = {}
        for r in chains:
            if r["status"] != "unmapped":
                per.setdefault((r["contig"], r["start"], r["end"], r["name"], r["block_id"], r["to_genome"]), []).append(r)
        mapped = [r for r in joined if r["status"] != "unmapped"]
        assert len(mapped) == len(per) > 10
        if joined_file == "g.block_lift_joined.tsv":          # (the planted indels lie at multiples of W: no window reaches across a chain break, BED intervals do)
            assert any(int(r["chains"]) > 1 for r in mapped) and any(int(r["chains"]) == 3 for r in mapped)
        for r in mapped:
            mine = per[(r["contig"], r["start"], r["end"], r["name"], r["block_id"], r["to_genome"])]
            assert int(r["chains"]) == len(mine) and (int(r["first_ch"]), int(r["last_ch"])) == (min(int(m["ch"]) for m in mine), max(int(m["ch"]) for m in mine)), r
            assert (int(r["src_start"]), int(r["src_end"])) == (min(int(m["src_start"]) for m in mine), max(int(m["src_end"]) for m in mine)), r
            assert (int(r["to_start"]), int(r["to_end"])) == (min(int(m["to_start"]) for m in mine), max(int(m["to_end"]) for m in mine)), r
            for f in COUNTS:
                assert int(r[f]) == sum(int(m[f]) for m in mine), (f, r)
            assert int(r["src_open_bases"]) == int(r["src_end"]) - int(r["src_start"]) - sum(int(m["src_end"]) - int(m["src_start"]) for m in mine), r
            assert int(r["to_open_bases"]) == int(r["to_end"]) - int(r["to_start"]) - sum(int(m["to_end"]) - int(m["to_start"]) for m in mine), r
        unmapped = {(r["contig"], r["start"], r["end"]) for r in joined if r["status"] == "unmapped"}
        assert unmapped == {(r["contig"], r["start"], r["end"]) for r in chains if r["status"] == "unmapped"}


def test_the_interval_across_the_planted_deletion_is_one_line_of_two_chains(runs):
    _, _, dirs, _, _ = runs
    _, joined = rows_of(dirs["joined"] / "g.block_lift_joined.tsv", assess.LIFT_JOINED_COLUMNS)
    across = [r for r in joined if r["name"] == "across_deletion" and r["to_genome"] == "fam2.fa"]
    assert len(across) == 1 and across[0]["chains"] == "2", across
    r = across[0]
    records = [p for p in records_of((dirs["joined"] / "g.block_alignments.paf").read_text())
               if p["block"] == r["block_id"] and {p["tg"], p["qg"]} == {SOURCE, "fam2.fa"} and p["ch"] in (int(r["first_ch"]), int(r["last_ch"]))]
    assert len(records) == 2
    first, last = sorted(records, key=lambda p: p["ch"])
    mine, other = (("t_from", "t_to"), ("q_from", "q_to")) if first["tg"] == SOURCE else (("q_from", "q_to"), ("t_from", "t_to"))

    def between(keys):                                        # the bases of one genome between the two records, whichever way the pair runs
        return max(first[keys[0]], last[keys[0]]) - min(first[keys[1]], last[keys[1]])
    assert int(r["src_open_bases"]) == between(mine) and int(r["to_open_bases"]) == between(other)
    assert int(r["src_open_bases"]) - int(r["to_open_bases"]) == between(mine) - between(other) > 0      # (genome 2 lacks bases there)


def test_with_wide_edits_and_ends_every_pair_is_one_chain(runs):
    _, _, dirs, _, _ = runs
    assert {len(p) for p in PB.paf_pairs((dirs["one_chain"] / "g.block_alignments.paf").read_text(), SOURCE)} == {1}
    for joined_file, chain_file in (("g.block_lift_joined.tsv", "g.block_lift_identity.tsv"), ("g.block_windows_joined.tsv", "g.block_windows.tsv")):
        _, joined = rows_of(dirs["one_chain"] / joined_file, assess.LIFT_JOINED_COLUMNS)
        _, chains = rows_of(dirs["one_chain"] / chain_file, assess.LIFT_IDENTITY_COLUMNS)
        assert len(joined) == len(chains) > 10
        for a, b in zip(joined, chains):
            assert [a[f] for f in assess.LIFT_COLUMNS[:11]] == [b[f] for f in assess.LIFT_COLUMNS[:11]], (a, b)
            assert [a[f] for f in ("src_start", "src_end") + COUNTS + ("columns", "identity", "status")] == \
                [b[f] for f in ("src_start", "src_end") + COUNTS + ("columns", "identity", "status")], (a, b)
            if a["status"] != "unmapped":
                assert (a["chains"], a["first_ch"], a["last_ch"], a["src_open_bases"], a["to_open_bases"]) == ("1", b["ch"], b["ch"], "0", "0")


def test_the_tool_reproduces_the_files(runs):
    tmp, paths, dirs, _, _ = runs
    fais = [str(dirs["joined"] / (os.path.basename(p) + ".fai")) for p in paths]
    common = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["joined"] / "g.synteny_blocks.tsv"), "--fai"] + fais + \
        ["--fastas"] + paths + ["--divergence-out", str(tmp / "tool.div.tsv"), "--lift-genome", SOURCE]
    # everything in one pass beside the PAF; then the joined tables alone (no per-chain call)
    r = _run(common + ["--paf-out", str(tmp / "tool.paf"), "--lift-bed", str(tmp / "iv.bed"), "--lift-out", str(tmp / "tool.lift.tsv"),
                       "--lift-identity-out", str(tmp / "tool.identity.tsv"), "--lift-windows", str(W), "--lift-windows-out", str(tmp / "tool.windows.tsv"),
                       "--lift-joined-out", str(tmp / "tool.joined.tsv"), "--lift-windows-joined-out", str(tmp / "tool.windows_joined.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    for mine, theirs in (("tool.paf", "g.block_alignments.paf"), ("tool.lift.tsv", "g.block_lift.tsv"), ("tool.identity.tsv", "g.block_lift_identity.tsv"),
                         ("tool.windows.tsv", "g.block_windows.tsv"), ("tool.joined.tsv", "g.block_lift_joined.tsv"),
                         ("tool.windows_joined.tsv", "g.block_windows_joined.tsv")):
        assert (tmp / mine).read_bytes() == (dirs["joined"] / theirs).read_bytes(), mine
    r = _run(common + ["--lift-bed", str(tmp / "iv.bed"), "--lift-joined-out", str(tmp / "tool.joined2.tsv"), "--lift-windows", str(W),
                       "--lift-windows-joined-out", str(tmp / "tool.windows_joined2.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.joined2.tsv").read_bytes() == (dirs["joined"] / "g.block_lift_joined.tsv").read_bytes()
    assert (tmp / "tool.windows_joined2.tsv").read_bytes() == (dirs["joined"] / "g.block_windows_joined.tsv").read_bytes()
    r = _run(common + ["--lift-joined-out", str(tmp / "no.tsv")], tmp)
    assert r.returncode == 2 and "--lift-joined-out needs the intervals" in r.stderr


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs, _, _ = runs
    same = sorted(os.listdir(dirs["without"]))
    assert "g.block_lift_identity.tsv" in same and "g.block_windows.tsv" in same and not [n for n in same if "joined" in n]
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["joined"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["joined"])) - set(same)) == ["g.block_lift_joined.tsv", "g.block_windows_joined.tsv"]
    stages = {d: [ln.split("\t")[0] for ln in (dirs[d] / "g.stage_times.tsv").read_text().splitlines()] for d in ("without", "joined")}
    new = [s for s in stages["joined"] if s.startswith("block_lift_joined")]
    assert new == ["block_lift_joined", "block_lift_joined:lift_pairs_scan", "block_lift_joined:lift_pairs_search"]
    assert [s for s in stages["joined"] if s not in new] == stages["without"]
    assert stages["joined"].index("block_lift_joined") > stages["joined"].index("block_windows")

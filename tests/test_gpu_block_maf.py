"""`ntSynt --block-maf` and `bin/ntsynt_block_stats --maf-out` end to end (ntsynt_amd/assess.py block_mafs; docs/design/04_29_block_maf.md)
on the family of tests/test_gpu_block_paf.py -- three genomes of 120 kbp with the planted indels -- run with --block-paf --block-maf
--identity-max-edits 1023 --block-ends --ends-max-len 1500, and again with E = 0 and no ends.  Every PAF record has exactly one MAF block,
in the same order; per block the degapped rows are the target and query substrings of the FASTA files (the query reverse-complemented for
`-`, its start converted back from the reverse strand), size is the number of non-gap bytes, the CIGAR of the two rows is the record's
own cg:Z:, score is the PAF's match count; --block-maf alone writes a byte-equal file; with the switch off every other file is
byte-equal; the planted 40-base deletion is exactly 40 `-` in row B of its block; the tool reproduces the file; --dry-run and --benchmark
list the stage and its timers; several ranks are refused at argument parsing.  Every test runs under a time limit of its own."""
import faulthandler
import os
import re
import sys

import pytest

from tests import extend_brute as X
from tests import maf_brute as MB
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import ENDS_MAX_LEN, MAX_EDITS, ROOT, SWITCHES, _run, paf_family, read_fasta, records_of

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
PAF, MAF = "g.block_alignments.paf", "g.block_alignments.maf"
WIDE = ["--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 1023 with ends without the switch, with it and with it alone; E = 0 without ends with --block-paf and alone"
    tmp = tmp_path_factory.mktemp("maf_runs")
    paths, _ = paf_family(str(tmp))
    dirs = {}
    for key, switches in (("without", SWITCHES + ["--block-paf"]), ("full", SWITCHES + ["--block-paf", "--block-maf"]), ("full_alone", WIDE + ["--block-maf"]),
                          ("narrow", ["--block-paf", "--block-maf"]), ("narrow_alone", ["--block-maf"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def test_every_paf_record_has_its_block_and_every_block_holds_the_fasta_bases(runs):
    _, paths, dirs = runs
    genomes = {os.path.basename(p): read_fasta(p) for p in paths}
    for key in ("full", "narrow"):
        records = records_of((dirs[key] / PAF).read_text())
        assert len(records) >= 6 and {r["sign"] for r in records} == {"+", "-"}
        for r in records:                                     # on this family every chain has a match column: checked, not assumed
            assert any(letter in "=X" for letter in re.findall(r"[=XID]", r["cg"])), r
        blocks = MB.parse_maf((dirs[key] / MAF).read_text())
        assert len(blocks) == len(records)
        gaps = 0
        for r, b in zip(records, blocks):
            assert (b["t_name"], b["q_name"]) == (f"{r['tg']}.{r['t']}", f"{r['qg']}.{r['q']}"), (r, b["t_name"], b["q_name"])
            target, query = genomes[r["tg"]][r["t"]], genomes[r["qg"]][r["q"]]
            assert (b["t_src_size"], b["q_src_size"], b["q_strand"], b["score"]) == (target.size, query.size, r["sign"], r["matches"])
            assert (b["t_start"], b["t_start"] + b["t_size"]) == (r["t_from"], r["t_to"])
            q_from = b["q_src_size"] - b["q_start"] - b["q_size"] if b["q_strand"] == "-" else b["q_start"]      # back from the reverse strand
            assert (q_from, q_from + b["q_size"]) == (r["q_from"], r["q_to"])
            row_a, row_b = b["t_row"], b["q_row"]
            assert len(row_a) == len(row_b) == r["columns"]
            assert b["t_size"] == len(row_a) - row_a.count("-") and b["q_size"] == len(row_b) - row_b.count("-")     # (size: the non-gap bytes)
            assert row_a.replace("-", "") == MB.letters(target[b["t_start"]:b["t_start"] + b["t_size"]])
            mine = query[q_from:q_from + b["q_size"]]
            assert row_b.replace("-", "") == MB.letters(X.revcomp(mine) if b["q_strand"] == "-" else mine)
            assert MB.cigar_of_rows(row_a, row_b) == r["cg"], (r["cg"][:100], MB.cigar_of_rows(row_a, row_b)[:100])
            gaps += row_a.count("-") + row_b.count("-")
        print(key, len(blocks), "blocks,", sum(len(b["t_row"]) for b in blocks), "columns,", gaps, "gap bytes")
        assert gaps > 100


def test_the_switch_alone_writes_the_same_file(runs):
    _, _, dirs = runs
    assert (dirs["full_alone"] / MAF).read_bytes() == (dirs["full"] / MAF).read_bytes()
    assert (dirs["narrow_alone"] / MAF).read_bytes() == (dirs["narrow"] / MAF).read_bytes()
    assert (dirs["narrow"] / MAF).read_bytes() != (dirs["full"] / MAF).read_bytes()
    assert not (dirs["narrow_alone"] / PAF).exists() and not (dirs["full_alone"] / PAF).exists()


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and "g.block_ends.tsv" in same and MAF not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == [MAF]
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "full")}
    assert [s for s in stages["full"] if s.startswith("block_maf")] == ["block_maf", "block_maf:cigar_rows_scan", "block_maf:cigar_rows_emit"]
    assert stages["full"].index("block_maf") > stages["full"].index("block_paf")
    assert [s for s in stages["full"] if not s.startswith("block_maf")] == stages["without"]


def test_the_planted_deletion_is_exactly_40_gap_bytes_in_row_b_of_its_block(runs):
    _, _, dirs = runs
    blocks = MB.parse_maf((dirs["full"] / MAF).read_text())
    # the deletion lies at base 50 000 of the record, give or take the few bases by which the indels planted further left shift it.  A
    # minimal script may spend its 40 gap columns among chance matches of the deleted bases with their neighbourhood (as the PAF test
    # notes for the insertions), so the gap bytes are counted over the columns of target bases 49 800 .. 50 300: the next planted indel
    # is at 45 000, and substitutions make no gap
    mine = [b for b in blocks if (b["t_name"], b["q_name"]) == ("fam0.fa.chr1", "fam2.fa.chr1") and b["t_start"] <= 49_800 and 50_300 <= b["t_start"] + b["t_size"]]
    assert len(mine) == 1
    b = mine[0]
    at, near_a, near_b = b["t_start"], [], []
    for ch_a, ch_b in zip(b["t_row"], b["q_row"]):
        if 49_800 <= at < 50_300:
            near_a.append(ch_a)
            near_b.append(ch_b)
        at += ch_a != "-"
    near_a, near_b = "".join(near_a), "".join(near_b)
    print("runs of - in row B near the deletion:", [(m.start(), len(m.group())) for m in re.finditer(r"-+", near_b)])
    assert near_b.count("-") == 40 and "-" not in near_a


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    out, alone = tmp / "tool.maf", tmp / "tool_alone.maf"
    r = _run(tool + ["--maf-out", str(out), "--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.ends.tsv"), "--ends-max-len", str(ENDS_MAX_LEN),
                     "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_bytes() == (dirs["full"] / MAF).read_bytes()
    r = _run(tool + ["--maf-out", str(alone), "--divergence-out", str(tmp / "tool.div2.tsv")], tmp)                 # E = 0, no ends, no other file
    assert r.returncode == 0, r.stderr[-3000:]
    assert alone.read_bytes() == (dirs["narrow"] / MAF).read_bytes()


def test_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _ = runs
    r = _run(NTSYNT + paths + PARAMS + WIDE + ["--block-maf", "--dry-run"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    listed = [ln for ln in (r.stdout + r.stderr).splitlines() if "block_maf (" in ln]
    assert len(listed) == 1 and "block_maf (cigar_rows_scan, cigar_rows_emit; k " in listed[0] and f"max_edits {MAX_EDITS}" in listed[0] and \
        f"ends_max_len {ENDS_MAX_LEN}" in listed[0], listed
    r = _run(NTSYNT + paths + PARAMS + ["--block-maf"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "--block-maf works from the genomes resident on one GPU" in r.stderr and "ntsynt_block_stats" in r.stderr and \
        "--maf-out" in r.stderr, r.stderr[-2000:]

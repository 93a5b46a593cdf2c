"""Block statistics (ntsynt_amd/assess.py block_stats, bin/ntsynt_block_stats) against what the reference's
analysis_scripts/denovo_synteny_block_stats.py prints for the same inputs (recorded under tests/golden/block_stats/*.expected.txt):
the four celegans block tables of tests/golden/ and three hand-written ones -- a block missing from one of three genomes, genomes of
unequal size, a single block.  Header byte-identical, integer columns equal, float columns within 1e-9 relative (double arithmetic
over a few thousand terms moves ~1e-12 with the order of summation; anything larger is a different rule)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "block_stats")
TOOL = os.path.join(ROOT, "bin", "ntsynt_block_stats")
CELEGANS3 = ["celegans-chrII-III.A.fa.fai", "celegans-chrII-III.B.fa.fai", "celegans-chrII-III.fa.fai"]
CELEGANS2 = ["celegans-chrII-III.A.fa.fai", "celegans-chrII-III.fa.fai"]
INPUTS = {
    "celegans-A-B-ntSynt.synteny_blocks": (GOLDEN, "celegans-A-B-ntSynt.synteny_blocks.tsv", CELEGANS3),
    "celegans-A-B-ntSynt.pre-collinear-merge.synteny_blocks": (GOLDEN, "celegans-A-B-ntSynt.pre-collinear-merge.synteny_blocks.tsv", CELEGANS3),
    "celegans-A-ntSynt.synteny_blocks": (GOLDEN, "celegans-A-ntSynt.synteny_blocks.tsv", CELEGANS2),
    "celegans-A-ntSynt.pre-collinear-merge.synteny_blocks": (GOLDEN, "celegans-A-ntSynt.pre-collinear-merge.synteny_blocks.tsv", CELEGANS2),
    "three_missing": (CASES, "three_missing.synteny_blocks.tsv", ["three_a.fa.fai", "three_b.fa.fai", "three_c.fa.fai"]),
    "unequal": (CASES, "unequal.synteny_blocks.tsv", ["unequal_big.fa.fai", "unequal_small.fa.fai"]),
    "single": (CASES, "single.synteny_blocks.tsv", ["single_x.fa.fai", "single_y.fa.fai"]),
}
INT_COLUMNS = {"Number_blocks", "Number_blocks_all_asm", "NG50_length", "N50_length"}


def _inputs(case):
    d, tsv, fais = INPUTS[case]
    return os.path.join(d, tsv), [os.path.join(d, f) for f in fais]


def _expected(case):
    header, line = open(os.path.join(CASES, case + ".expected.txt"), encoding="utf-8").read().splitlines()
    return header, line.split("\t")


def _same(header, line, case):
    exp_header, exp = _expected(case)
    assert header == exp_header
    names, got = header.split("\t"), line.split("\t")
    assert len(names) == 10 and len(got) == 10
    for name, g, e in zip(names, got, exp):
        if name in INT_COLUMNS:
            assert g == e, (case, name, g, e)
        else:
            assert abs(float(g) - float(e)) <= 1e-9 * abs(float(e)), (case, name, g, e)


@pytest.mark.parametrize("case", sorted(INPUTS))
def test_block_stats_match_the_reference_script(case):
    from ntsynt_amd import assess
    tsv, fais = _inputs(case)
    stats = assess.block_stats(tsv, fais)
    assert tuple(stats) == assess.STATS_COLUMNS
    header, line = assess.stats_table(stats).splitlines()
    _same(header, line, case)


def test_the_figures_quoted_for_the_celegans_tables():
    from ntsynt_amd import assess
    ab = assess.block_stats(*_inputs("celegans-A-B-ntSynt.synteny_blocks"))
    a = assess.block_stats(*_inputs("celegans-A-ntSynt.synteny_blocks"))
    assert (ab["Number_blocks"], ab["NG50_length"]) == (15, 4273546)
    assert (a["Number_blocks"], a["NG50_length"]) == (11, 4842145)


def test_hand_written_cases_exercise_what_they_were_written_for():
    from ntsynt_amd import assess
    m = assess.block_stats(*_inputs("three_missing"))
    assert m["Number_blocks"] != m["Number_blocks_all_asm"] and m["Average_coverage"] != m["Average_coverage_all_asm"]
    u = assess.block_stats(*_inputs("unequal"))
    tsv, fais = _inputs("unequal")
    small = sum(r.end - r.start for r in assess.read_blocks(tsv) if r.genome == "unequal_small.fa")
    assert u["Coverage_min_genome_size"] == small / 42000 * 100                  # the smaller genome's side
    assert assess.block_stats(*_inputs("single"))["Number_blocks"] == 1


def test_read_blocks_columns():
    from ntsynt_amd import assess
    rows = assess.read_blocks(_inputs("celegans-A-B-ntSynt.synteny_blocks")[0])
    assert len(rows) == 45
    r = rows[0]
    assert (r.block_id, r.genome, r.contig, r.start, r.end, r.strand, r.minimizers, r.reason) == \
        ("0", "celegans-chrII-III.A.fa", "gi|453231901|ref|NC_003280.10|", 170, 1729744, "+", "2866", "None")


@pytest.mark.parametrize("case", ["celegans-A-B-ntSynt.synteny_blocks", "three_missing"])
def test_tool_prints_the_same_line_and_does_not_import_torch(case, tmp_path):
    tsv, fais = _inputs(case)
    r = subprocess.run([sys.executable, "-X", "importtime", TOOL, "--tsv", tsv, "--fai"] + fais, capture_output=True, text=True, timeout=120,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    header, line = r.stdout.splitlines()
    _same(header, line, case)
    imported = {ln.rsplit("|", 1)[1].strip() for ln in r.stderr.splitlines() if ln.startswith("import time:") and "|" in ln}
    assert "os" in imported or "re" in imported                                 # (the listing is there)
    assert not [m for m in imported if m == "torch" or m.startswith("torch.")], "the statistics must not import torch"


def test_divergence_table_rendering():
    from ntsynt_amd import assess
    rows = [{"block_id": "0", "genome_a": "a.fa", "genome_b": "b.fa", "distance": 0.0123456789, "shared_hashes": 7, "sketch_size": 10,
             "kmers_a": 100, "kmers_b": 90}]
    assert assess.divergence_table(rows, 21, 1000) == ("block_id\tgenome_a\tgenome_b\tdistance\tshared_hashes\tsketch_size\tkmers_a\tkmers_b\n"
                                                       "0\ta.fa\tb.fa\t0.0123457\t7\t10\t100\t90\n# k 21, sketch 1000\n")


def test_assess_switch_on_the_command_line(capsys, monkeypatch, tmp_path):
    from ntsynt_amd import cli
    fa = [str(tmp_path / "a.fa"), str(tmp_path / "b.fa")]
    for p in fa:
        open(p, "w").write(">x\nACGT\n")
    assert cli.main(fa + ["-d", "1", "-n", "--assess"]) == 0
    assert capsys.readouterr().out.rstrip().endswith("ntsynt_synteny -> assess")
    assert cli.main(fa + ["-d", "1", "-n"]) == 0
    assert capsys.readouterr().out.rstrip().endswith("ntsynt_synteny")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as exc:
        cli.main(fa + ["-d", "1", "--assess"])
    assert exc.value.code == 2 and "--assess works from the genomes resident on one GPU" in capsys.readouterr().err

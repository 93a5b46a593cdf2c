"""`ntSynt --block-ends` and `bin/ntsynt_block_stats --ends-out` end to end (ntsynt_amd/assess.py block_ends;
docs/design/04_20_block_ends.md): three genomes of 2 x 60 kbp at 1 % substitutions; genome 1 has 8 kbp of its first record inverted,
genome 2 has the last 5 kbp of its second record replaced by unrelated sequence, genome 0 has a run of 300 N in its second record,
1 000 bases behind the end of the last block.  On the CPU first (tests/extend_brute.py over the flanks rebuilt from the segments of
tests/identity_brute.py on the oracle's hashes): at the three planted junctions the extended ends lie within 16 bases of the planted
coordinate with stop `break`, in `+` and in `-` pairs; the flank that faces the N run stops `invalid` at its first N; flanks reach both
ends of a record and stop `record`; the pairs that do not hold a junction run on to `max_len`.  Then the runs: the file equals the
recomputation byte for byte, the tool reproduces it, every other file is the plain run's, without the switch nothing of it exists, and
several ranks are refused.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, synth
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import extend_brute as X
from tests import identity_brute as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
PARAMS = ["-d", "1", "-k", "24", "-w", "100", "--w_rounds", "50", "10", "--indel", "500", "--merge", "1000", "-b", "2000", "-p", "g"]
ORACLE = dict(prefix="g", k=24, w=100, w_rounds=(50, 10), indel=500, merge=1000, block_size=2000)
K, RATE, BAND, MAX_LEN, MAX_EDITS = 21, 16, 31, 4096, 0      # the identity switches' defaults
ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY = 1500, 255, 6    # (1 500 bases: the brute force's tables stay small; the other two are the defaults)
ENDS = ["--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
INVERT_AT, INVERT_END = 24_000, 32_000                        # genome 1, record 1
UNRELATED_FROM = 55_000                                       # genome 2, record 2: unrelated from here to the record's end
N_AT, N_BASES = 56_000, 300                                   # genome 0, record 2
NEAR = 16


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def ends_family(outdir):
    "(paths, genomes)"
    anc = synth.make_ancestor(120_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(121)
    c = fam[1][0]
    c[INVERT_AT:INVERT_END] = synth.revcomp(c[INVERT_AT:INVERT_END])
    fam[2][1][UNRELATED_FROM:] = synth.random_dna(fam[2][1].size - UNRELATED_FROM, rng)
    fam[0][1][N_AT:N_AT + N_BASES] = ord("N")
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def recompute(blocks_tsv, fam, names):
    "(text, {(block, genome a, genome b): the pair's columns}) from the brute forces alone: no GPU, none of assess.block_ends"
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    table = assess.read_blocks(blocks_tsv)
    _, facts = B.brute_file(table, genomes, O.hash_all, K, RATE, BAND, MAX_LEN)
    return X.ends_file(table, genomes, facts, K, RATE, BAND, MAX_LEN, MAX_EDITS, ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY)


def rows_of(text):
    "[{column: field}] of an ends table"
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert tuple(head) == assess.ENDS_COLUMNS
    return [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def check_the_planted_facts(text):
    "what a table must show of the family; asserted on the recomputation before any GPU run is looked at"
    rows = rows_of(text)
    assert text.splitlines()[-1] == (f"# k {K}, rate {RATE}, band {BAND}, max_len {MAX_LEN}, max_edits {MAX_EDITS}, ends_max_len {ENDS_MAX_LEN}, "
                                     f"ends_max_edits {ENDS_MAX_EDITS}, ends_penalty {ENDS_PENALTY}")
    assert all(r["left_stop"] != "." for r in rows), "a pair without an aligned segment"
    seen = set()
    for r in rows:
        with_1 = "fam1.fa" in (r["genome_a"], r["genome_b"])
        with_2 = "fam2.fa" in (r["genome_a"], r["genome_b"])
        flipped = r["orientation"] == "-"
        for side, ext in (("left", "ext_start"), ("right", "ext_end")):
            at_a, at_b, stop = int(r[ext + "_a"]), int(r[ext + "_b"]), r[side + "_stop"]
            end_b = int(r["ext_end_b" if (side == "left") == flipped else "ext_start_b"]) if flipped else at_b
            for planted in (INVERT_AT, INVERT_END):          # the two junctions of the inversion, in every pair that holds genome 1
                mirrored = INVERT_AT + INVERT_END - planted if flipped else planted     # (where genome 1 holds that junction's other side)
                if r["contig_a"] == "chr1" and with_1 and abs(at_a - planted) <= 2000:
                    assert stop == "break" and abs(at_a - planted) <= NEAR and abs(end_b - mirrored) <= NEAR, (r, side, planted)
                    seen.add(("junction", planted, r["orientation"]))
            if r["contig_a"] == "chr2" and side == "right":
                if with_2:                                    # the unrelated tail of genome 2
                    assert stop == "break" and abs(at_a - UNRELATED_FROM) <= NEAR and abs(at_b - UNRELATED_FROM) <= NEAR, (r, side)
                    seen.add(("junction", UNRELATED_FROM, r["orientation"]))
                else:                                         # genomes 0 and 1 go on together up to the first N
                    assert stop == "invalid" and at_a == N_AT and abs(at_b - N_AT) <= NEAR, (r, side)
                    seen.add("invalid")
            if stop == "record":
                assert (at_a, at_b) == ((0, 0) if side == "left" else (60_000, 60_000)), (r, side)
                seen.add(("record", side))
            if stop == "max_len":                             # a pair that does not hold the junction's genome runs across it
                assert not with_1 and r["contig_a"] == "chr1" and int(r[side + "_a"]) == ENDS_MAX_LEN and int(r[side + "_edits"]) >= 5, (r, side)
                seen.add("max_len")
    want = {("junction", INVERT_AT, "+"), ("junction", INVERT_AT, "-"), ("junction", INVERT_END, "+"), ("junction", INVERT_END, "-"),
            ("junction", UNRELATED_FROM, "+"), "invalid", ("record", "left"), ("record", "right"), "max_len"}
    assert seen == want, (want - seen, seen - want)


def _run(cmd, cwd, **env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT, **env))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table and the recomputation (checked before any GPU run), two runs: plain and with the switch"
    tmp = tmp_path_factory.mktemp("ends_runs")
    paths, fam = ends_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    (tmp / "oracle" / "table.tsv").write_text(table)
    text, _ = recompute(str(tmp / "oracle" / "table.tsv"), fam, [os.path.basename(p) for p in paths])
    check_the_planted_facts(text)
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("plain", ["--benchmark"]), ("ends", ENDS + ["--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["ends"] / "g.synteny_blocks.tsv").read_text() == table
    return tmp, paths, dirs, text


def test_the_file_equals_the_recomputation(runs):
    _, _, dirs, text = runs
    got = (dirs["ends"] / "g.block_ends.tsv").read_text()
    check_the_planted_facts(got)
    assert {r["orientation"] for r in rows_of(got)} == {"+", "-"}
    assert got == text


def test_every_other_file_is_the_plain_run_s_and_nothing_of_it_exists_without_the_switch(runs):
    _, _, dirs, _ = runs
    same = sorted(os.listdir(dirs["plain"]))
    assert "g.synteny_blocks.tsv" in same and not [n for n in same if "block_ends" in n]
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["plain"] / name).read_bytes() == (dirs["ends"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["ends"])) - set(same)) == ["g.block_ends.tsv"]
    stages = {name: [ln.split("\t")[0] for ln in (dirs[name] / "g.stage_times.tsv").read_text().splitlines()] for name in dirs}
    assert "block_ends" in stages["ends"] and "block_ends:edit_extend" in stages["ends"]
    assert not [s for s in stages["plain"] if "block_ends" in s or "edit_extend" in s]
    assert [s for s in stages["ends"] if "block_ends" not in s] == stages["plain"]


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs, text = runs
    out = tmp / "tool.block_ends.tsv"
    fais = [str(dirs["ends"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["ends"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["ends"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--ends-out", str(out), "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text


def test_the_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _, _ = runs
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    r = _run(ntsynt + paths + PARAMS + ENDS + ["--dry-run"], tmp)
    assert r.returncode == 0 and "block_ends (edit_extend)" in r.stdout + r.stderr, r.stderr[-2000:]
    r = _run(ntsynt + paths + PARAMS + ["--dry-run"], tmp)
    assert r.returncode == 0 and "edit_extend" not in r.stdout + r.stderr
    r = _run(ntsynt + paths + PARAMS + ENDS + ["--dry-run"], tmp, WORLD_SIZE="2")
    assert r.returncode != 0 and "--block-ends works from the genomes resident on one GPU" in r.stderr, r.stderr[-2000:]
    for bad in (["--ends-max-len", "0"], ["--ends-max-edits", "1024"], ["--ends-penalty", "2"]):
        r = _run(ntsynt + paths + PARAMS + ["--block-ends"] + bad + ["--dry-run"], tmp)
        assert r.returncode != 0 and bad[0] in r.stderr, (bad, r.stderr[-2000:])

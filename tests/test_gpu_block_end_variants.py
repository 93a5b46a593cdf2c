"""`ntSynt --block-ends --block-end-variants` and `bin/ntsynt_block_stats --ends-out F --end-variants-out G` end to end
(ntsynt_amd/assess.py block_ends with_variants; docs/design/04_21_block_end_variants.md): the family of tests/test_gpu_block_ends.py
-- three genomes of 2 x 60 kbp at 1 % substitutions, 8 kbp of genome 1's first record inverted, an unrelated tail in genome 2, a run of
N in genome 0 -- with a second inversion in genome 1's second record, genome 2's whole second record reverse-complemented (the pair of
genomes 0 and 2 is `-` there) and, in genome 2, a deletion and an insertion of 15 and 14 bases just inside either end of both inverted
spans: the flanks of the pair (0, 2), which run on across genome 1's junctions, cross them.  On the CPU first
(tests/end_variants_brute.py on the segments of tests/identity_brute.py over the oracle's hashes): the recomputed file holds an `ins`
and a `del` of 5 bases or more in a left flank and in a right flank, in a `+` pair and in a `-` pair.  Then the runs: the file equals
the recomputation byte for byte; per flank the summed lengths of its events are left_edits / right_edits of block_ends.tsv; applying a
flank's events to A's interval gives B's oriented interval; block_ends.tsv and every other file are those of a run with --block-ends
alone, in which the new file does not exist; the tool reproduces the file.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, synth
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import end_variants_brute as EB
from tests import extend_brute as X
from tests import identity_brute as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
PARAMS = ["-d", "1", "-k", "24", "-w", "100", "--w_rounds", "50", "10", "--indel", "500", "--merge", "1000", "-b", "2000", "-p", "g"]
ORACLE = dict(prefix="g", k=24, w=100, w_rounds=(50, 10), indel=500, merge=1000, block_size=2000)
K, RATE, BAND, MAX_LEN, MAX_EDITS = 21, 16, 31, 4096, 0      # the identity switches' defaults
ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY = 1500, 255, 6
ENDS = ["--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
SPANS = ((0, 24_000, 32_000), (1, 20_000, 28_000))            # genome 1: (record, start, end) of its two inversions
UNRELATED_FROM = 55_000                                       # genome 2, record 2 (before it is reverse-complemented)
N_AT, N_BASES = 56_000, 300                                   # genome 0, record 2
DELETED, INSERTED = 15, 14


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def variants_family(outdir):
    "(paths, genomes)"
    anc = synth.make_ancestor(120_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(121)
    for rec, lo, hi in SPANS:
        fam[1][rec][lo:hi] = synth.revcomp(fam[1][rec][lo:hi])
    fam[2][1][UNRELATED_FROM:] = synth.random_dna(fam[2][1].size - UNRELATED_FROM, rng)
    fam[0][1][N_AT:N_AT + N_BASES] = ord("N")
    for rec, lo, hi in SPANS:                                 # genome 2: from the right, so that the earlier positions hold
        c = fam[2][rec]
        for at, deleted in ((hi - 350, False), (hi - 800, True), (lo + 800, False), (lo + 350, True)):
            c = np.concatenate([c[:at], c[at + DELETED:]]) if deleted else np.concatenate([c[:at], synth.random_dna(INSERTED, rng), c[at:]])
        fam[2][rec] = c
    fam[2][1] = synth.revcomp(fam[2][1])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def recompute(blocks_tsv, fam, names):
    "(the variants text, the ends text) from the brute forces alone: no GPU, none of assess.block_ends"
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    table = assess.read_blocks(blocks_tsv)
    _, facts = B.brute_file(table, genomes, O.hash_all, K, RATE, BAND, MAX_LEN)
    args = (K, RATE, BAND, MAX_LEN, MAX_EDITS, ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY)
    return EB.end_variants_file(table, genomes, facts, *args)[0], X.ends_file(table, genomes, facts, *args)[0]


def rows_of(text, columns):
    lines = text.splitlines()
    assert tuple(lines[0].split("\t")) == tuple(columns) and lines[-1].startswith("# k ")
    return [dict(zip(columns, ln.split("\t"))) for ln in lines[1:-1]]


def check_the_planted_condition(text):
    "an `ins` and a `del` of 5 bases or more in a left flank and in a right flank, in a `+` pair and in a `-` pair"
    rows = rows_of(text, EB.COLUMNS)
    seen = {(r["type"], r["flank"], r["orientation"]) for r in rows if r["type"] != "snv" and int(r["length"]) >= 5}
    want = {(kind, flank, sign) for kind in ("ins", "del") for flank in ("left", "right") for sign in "+-"}
    assert seen >= want, want - seen
    assert {r["type"] for r in rows} == {"snv", "ins", "del"}


def _run(cmd, cwd, **env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT, **env))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table and the recomputation (its condition checked before any GPU run), two runs: --block-ends alone and with the switch"
    tmp = tmp_path_factory.mktemp("end_variant_runs")
    paths, fam = variants_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    (tmp / "oracle" / "table.tsv").write_text(table)
    text, ends_text = recompute(str(tmp / "oracle" / "table.tsv"), fam, [os.path.basename(p) for p in paths])
    check_the_planted_condition(text)
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("ends", ENDS + ["--benchmark"]), ("variants", ENDS + ["--block-end-variants", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["variants"] / "g.synteny_blocks.tsv").read_text() == table
    return tmp, paths, fam, dirs, text, ends_text


def test_the_file_equals_the_recomputation(runs):
    _, _, _, dirs, text, ends_text = runs
    got = (dirs["variants"] / "g.block_end_variants.tsv").read_text()
    check_the_planted_condition(got)
    assert got == text
    assert (dirs["variants"] / "g.block_ends.tsv").read_text() == ends_text


def test_the_events_of_a_flank_add_up_to_its_edits_and_turn_a_into_b(runs):
    _, paths, fam, dirs, _, _ = runs
    names = [os.path.basename(p) for p in paths]
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    ends = rows_of((dirs["variants"] / "g.block_ends.tsv").read_text(), assess.ENDS_COLUMNS)
    events = rows_of((dirs["variants"] / "g.block_end_variants.tsv").read_text(), assess.END_VARIANT_COLUMNS)
    checked = 0
    for e in ends:
        assert e["left_edits"] != "."
        seq_a, seq_b = genomes[e["genome_a"]][e["contig_a"]], genomes[e["genome_b"]][e["contig_b"]]
        flipped = e["orientation"] == "-"
        frame_b = X.revcomp(seq_b) if flipped else seq_b
        lo_b, hi_b = int(e["ext_start_b"]), int(e["ext_end_b"])
        if flipped:
            lo_b, hi_b = seq_b.size - hi_b, seq_b.size - lo_b
        lo_a, hi_a = int(e["ext_start_a"]), int(e["ext_end_a"])
        for side, a_from, a_to, b_from, b_to in (("left", lo_a, lo_a + int(e["left_a"]), lo_b, lo_b + int(e["left_b"])),
                                                 ("right", hi_a - int(e["right_a"]), hi_a, hi_b - int(e["right_b"]), hi_b)):
            mine = [v for v in events if (v["block_id"], v["genome_a"], v["genome_b"], v["flank"]) == (e["block_id"], e["genome_a"], e["genome_b"], side)]
            assert sum(int(v["length"]) for v in mine) == int(e[side + "_edits"]), (e, side)
            out, at = [], a_from
            for v in mine:
                pos_a = int(v["pos_a"])
                assert at <= pos_a <= a_to, (v, at)
                out.append(seq_a[at:pos_a].tobytes().decode())
                bases_a = "" if v["seq_a"] == "-" else v["seq_a"]
                assert seq_a[pos_a:pos_a + len(bases_a)].tobytes().decode() == bases_a, v
                out.append("" if v["seq_b"] == "-" else v["seq_b"])
                at = pos_a + len(bases_a)
            out.append(seq_a[at:a_to].tobytes().decode())
            assert "".join(out) == frame_b[b_from:b_to].tobytes().decode(), (e, side)
            checked += bool(mine)
    assert checked >= 8


def test_every_other_file_is_that_of_block_ends_alone(runs):
    _, _, _, dirs, _, _ = runs
    same = sorted(os.listdir(dirs["ends"]))
    assert "g.block_ends.tsv" in same and not [n for n in same if "end_variants" in n]
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["ends"] / name).read_bytes() == (dirs["variants"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["variants"])) - set(same)) == ["g.block_end_variants.tsv"]
    stages = {name: [ln.split("\t")[0] for ln in (dirs[name] / "g.stage_times.tsv").read_text().splitlines()] for name in dirs}
    assert "block_ends:edit_extend_script" in stages["variants"] and "block_ends:edit_extend_script_plan" in stages["variants"]
    assert not [s for s in stages["ends"] if "edit_extend_script" in s]
    assert [s for s in stages["variants"] if "edit_extend_script" not in s] == stages["ends"]


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, _, dirs, text, ends_text = runs
    out, ends_out = tmp / "tool.block_end_variants.tsv", tmp / "tool.block_ends.tsv"
    fais = [str(dirs["variants"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["variants"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["variants"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--ends-out", str(ends_out), "--end-variants-out", str(out), "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out",
                                     str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text and ends_out.read_text() == ends_text

"""`ntSynt --block-identity --identity-max-edits E` and `bin/ntsynt_block_stats --identity-out ... --identity-max-edits E` end to end
(ntsynt_amd/assess.py block_identity with max_edits; docs/design/04_18_block_identity_wide.md): the three genomes of 2 x 60 kbp at 1 %
with an 8 kbp inverted stretch in genome 1 of tests/test_gpu_block_variants.py, and in genome 2 two insertions and two deletions of
40, 150, 400 and 900 bases, two of them inside the inverted stretch.  On the CPU first (tests/wide_brute.py on the oracle's hashes):
without E some pair has offband segments, with E = 1023 it has none and its edits grow by at least the length differences of the
segments that were offband, planted lengths among them.  Then the runs: the file with E equals the recomputation byte for byte, the
tool reproduces it, every other file is the plain run's, and the file without the switch is the one of the band alone, footer
included.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, synth
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import identity_brute as B
from tests import wide_brute as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
PARAMS = ["-d", "1", "-k", "24", "-w", "100", "--w_rounds", "50", "10", "--indel", "500", "--merge", "1000", "-b", "2000", "-p", "g"]
ORACLE = dict(prefix="g", k=24, w=100, w_rounds=(50, 10), indel=500, merge=1000, block_size=2000)
K, RATE, BAND, MAX_LEN = 21, 16, 31, 4096                    # the switches' defaults
MAX_EDITS = 1023
INVERT_AT, INVERT_BP = 24_000, 8_000                         # genome 1, contig 1: the oracle reports it as a block
# genome 2: (contig, position in the unedited contig, bases inserted (+) or deleted (-)); the first two lie inside the inverted stretch
INDELS = [(0, 26_000, 40), (0, 29_500, -150), (1, 20_000, 400), (1, 40_000, -900)]


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def wide_family(outdir):
    "(paths, genomes)"
    anc = synth.make_ancestor(120_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(34)
    for contig in (0, 1):
        c = fam[2][contig]
        pieces, at = [], 0
        for _, where, n in [x for x in INDELS if x[0] == contig]:
            pieces.append(c[at:where])
            if n > 0:
                pieces.append(synth.random_dna(n, rng))
                at = where
            else:
                at = where - n
        fam[2][contig] = np.concatenate(pieces + [c[at:]])
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def recompute(blocks_tsv, fam, names):
    "(text with E, facts with E, text without E) of tests/wide_brute.py over a block table: no GPU, none of assess.block_identity"
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    return W.brute_file_wide(assess.read_blocks(blocks_tsv), genomes, O.hash_all, K, RATE, BAND, MAX_LEN, MAX_EDITS)


def rows_of(text):
    "{(block, genome a, genome b): {column: field}} of an identity table"
    lines = text.splitlines()
    head = lines[0].split("\t")
    return {tuple(ln.split("\t")[:3]): dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]}


def check_on_the_cpu(text, facts, narrow_text):
    "what the recomputation must show before any GPU run is looked at; returns the pairs that had offband segments"
    narrow, wide = rows_of(narrow_text), rows_of(text)
    assert narrow.keys() == wide.keys() and narrow_text.splitlines()[-1] == f"# k {K}, rate {RATE}, band {BAND}, max_len {MAX_LEN}"
    assert text.splitlines()[-1] == narrow_text.splitlines()[-1] + f", max_edits {MAX_EDITS}"
    had = [key for key, r in narrow.items() if int(r["offband"]) > 0]
    assert had, "no pair has an offband segment without E: the planted indels fell outside the blocks"
    gaps_seen, flipped = set(), 0
    for key in had:
        row, results = facts[key]
        rescued = [abs(seg[4] - seg[2]) for seg, d in results if seg[5] == B.OFFBAND and d < B.INVALID]
        gaps_seen |= set(rescued)
        flipped += row["orientation"] == "-"
        grown = row["edits"] - int(narrow[key]["edits"])
        print(f"block {key[0]} {key[1]} {key[2]} {row['orientation']}: offband {narrow[key]['offband']} -> {row['offband']}, edits "
              f"{narrow[key]['edits']} -> {row['edits']}, length differences of the rescued segments {rescued}")
        assert row["offband"] == 0 and int(wide[key]["offband"]) == 0, key
        assert rescued and grown >= sum(rescued), key
        assert row["aligned"] > int(narrow[key]["aligned"]) and row["aligned_a"] > int(narrow[key]["aligned_a"])
    planted = {abs(n) for _, _, n in INDELS}
    assert len(gaps_seen & planted) >= 2, (gaps_seen, "fewer than two planted indels lie whole between two anchors")
    assert flipped >= 1, "no pair of differing strands had an offband segment"
    for key in narrow.keys() - set(had):                      # a pair without offband or overband segments keeps its line
        if int(narrow[key]["overband"]) == 0:
            assert narrow[key] == wide[key], key
    return had


def _run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table and the recomputation (checked before any GPU run), three runs: plain, the band alone, with E"
    tmp = tmp_path_factory.mktemp("block_identity_wide")
    paths, fam = wide_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    (tmp / "oracle" / "table.tsv").write_text(table)
    text, facts, narrow_text = recompute(str(tmp / "oracle" / "table.tsv"), fam, [os.path.basename(p) for p in paths])
    had = check_on_the_cpu(text, facts, narrow_text)
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("plain", []), ("narrow", ["--block-identity"]),
                        ("wide", ["--block-identity", "--identity-max-edits", str(MAX_EDITS), "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["wide"] / "g.synteny_blocks.tsv").read_text() == table
    return tmp, paths, dirs, text, narrow_text, had


def test_the_file_with_e_equals_the_recomputation(runs):
    _, _, dirs, text, _, had = runs
    got = (dirs["wide"] / "g.block_identity.tsv").read_text()
    got_rows = rows_of(got)
    for key in had:
        assert int(got_rows[key]["offband"]) == 0, key
    assert got == text


def test_without_the_switch_the_file_is_the_band_s(runs):
    _, _, dirs, _, narrow_text, had = runs
    got = (dirs["narrow"] / "g.block_identity.tsv").read_text()
    assert got == narrow_text and got.splitlines()[-1] == f"# k {K}, rate {RATE}, band {BAND}, max_len {MAX_LEN}"
    assert all(int(rows_of(got)[key]["offband"]) > 0 for key in had)


def test_every_other_file_is_the_plain_run_s(runs):
    _, _, dirs, _, _, _ = runs
    same = sorted(os.listdir(dirs["plain"]))
    assert "g.synteny_blocks.tsv" in same
    for name in same:
        assert (dirs["plain"] / name).read_bytes() == (dirs["wide"] / name).read_bytes() == (dirs["narrow"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["narrow"])) - set(same)) == ["g.block_identity.tsv"]
    assert sorted(set(os.listdir(dirs["wide"])) - set(same)) == ["g.block_identity.tsv", "g.stage_times.tsv"]
    stages = [ln.split("\t")[0] for ln in (dirs["wide"] / "g.stage_times.tsv").read_text().splitlines()]
    assert "block_identity" in stages and "block_identity:edit_wide_plan" in stages and "block_identity:edit_wide" in stages


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs, text, _, _ = runs
    out = tmp / "tool.block_identity.tsv"
    fais = [str(dirs["wide"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["wide"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["wide"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--identity-out", str(out), "--identity-max-edits", str(MAX_EDITS), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text

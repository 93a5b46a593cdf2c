"""`ntSynt --block-identity` and `bin/ntsynt_block_stats --identity-out` end to end (ntsynt_amd/assess.py block_identity;
docs/design/04_16_block_identity.md): the three-genome family of the gap tests (2 x 300 kbp at 1 %) with a 30 kbp inverted segment in
genome 1 -- long enough for a block of its own whose lines differ in strand, which the CPU oracle's table must show -- and eight
indels of 1 - 20 bases in genome 2's second contig.  The file is recomputed byte for byte on the CPU (tests/identity_brute.py: the
oracle's hashes, dictionaries, the full edit-distance table); every other file of the run is what it is without the switch; the tool
gives the same bytes; a contig that differs by substitutions only has no segment off the main diagonal and no more edits than
substitutions; the contig with the indels has aligned segments off it; the inverted block's identity is the family's, not a random
pair's.  Every test runs under a time limit of its own."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
PARAMS = ["-d", "1", "-k", "24", "-w", "300", "--w_rounds", "100", "10", "--indel", "500", "--merge", "1000", "-b", "8000", "-p", "g"]
ORACLE = dict(prefix="g", k=24, w=300, w_rounds=(100, 10), indel=500, merge=1000, block_size=8000)
K, RATE, BAND, MAX_LEN = 21, 16, 31, 4096                    # the switches' defaults
INVERT_AT, INVERT_BP = 180_000, 30_000                       # genome 1, contig 1; chosen on the CPU: the oracle reports it as a block
N_INDELS = 8                                                 # genome 2, contig 2


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def identity_family(outdir):
    "(paths, genomes, the indels as (position in genome 2's contig 2, bases inserted (+) or deleted (-)))"
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    rng = np.random.default_rng(33)
    c = fam[2][1]
    pieces, at, indels = [], 0, []
    for where in sorted(rng.choice(np.arange(20_000, 280_000, 5_000), size=N_INDELS, replace=False).tolist()):
        n = int(rng.integers(1, 21))
        pieces.append(c[at:where])
        if rng.random() < 0.5:
            pieces.append(synth.random_dna(n, rng))
            at = where
            indels.append((where, n))
        else:
            at = where + n
            indels.append((where, -n))
    fam[2][1] = np.concatenate(pieces + [c[at:]])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam, indels


def recompute(blocks_tsv, fam, names):
    "(text, facts) of tests/identity_brute.py over a block table: no GPU, none of assess.block_identity"
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    return B.brute_file(assess.read_blocks(blocks_tsv), genomes, O.hash_all, K, RATE, BAND, MAX_LEN)


def _run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table (checked before any GPU run), two runs -- plain and with the switch -- and the recomputation"
    tmp = tmp_path_factory.mktemp("block_identity")
    paths, fam, indels = identity_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    strands = {}
    for ln in table.splitlines():
        f = ln.split("\t")
        strands.setdefault(f[0], set()).add(f[5])
    assert any(len(s) == 2 for s in strands.values()), "the oracle's table has no block whose lines differ in strand: lengthen the inversion"
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("plain", []), ("identity", ["--block-identity", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["identity"] / "g.synteny_blocks.tsv").read_text() == table
    text, facts = recompute(str(dirs["identity"] / "g.synteny_blocks.tsv"), fam, [os.path.basename(p) for p in paths])
    return tmp, paths, fam, indels, dirs, text, facts


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, _, _, dirs, _, _ = runs
    plain, with_id = dirs["plain"], dirs["identity"]
    same = sorted(os.listdir(plain))
    assert "g.synteny_blocks.tsv" in same
    for name in same:
        assert (plain / name).read_bytes() == (with_id / name).read_bytes() and (plain / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_id)) - set(same)) == ["g.block_identity.tsv", "g.stage_times.tsv"]
    stages = [ln.split("\t")[0] for ln in (with_id / "g.stage_times.tsv").read_text().splitlines()]
    assert "block_identity" in stages


def test_the_file_equals_the_recomputation(runs):
    _, _, _, _, dirs, text, facts = runs
    got = (dirs["identity"] / "g.block_identity.tsv").read_text()
    rows = [r for r, _ in facts.values()]
    print(f"{len(rows)} pairs, {sum(r['anchors'] for r in rows)} anchors, {sum(r['aligned'] for r in rows)} aligned segments, "
          f"{sum(r['edits'] for r in rows)} edits; kinds: " + ", ".join(f"{n} {sum(r[n] for r in rows)}" for n in ("backward", "long", "offband", "invalid", "overband")))
    assert sum(r["aligned"] for r in rows) > 10_000
    assert got == text


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, _, _, dirs, text, _ = runs
    out = tmp / "tool.block_identity.tsv"
    fais = [str(dirs["identity"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["identity"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["identity"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--identity-out", str(out), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text


def test_substitutions_indels_and_the_inverted_block(runs):
    _, _, fam, indels, _, _, facts = runs
    blocks_of = {}
    for (b, ga, gb), (row, segs) in facts.items():
        blocks_of.setdefault(b, []).append((ga, gb, row, segs))
    # substitutions only: genomes 0 and 1 over contig 2 (no indel, no inversion there): every segment on the main diagonal, and no
    # more edits than the substitutions planted between the two genomes inside the aligned stretches (Hamming bounds Levenshtein)
    _, _, _, _, dirs, _, _ = runs
    a, c = fam[0][1], fam[1][1]
    starts = {(r.block_id, r.genome): r.start for r in assess.read_blocks(str(dirs["identity"] / "g.synteny_blocks.tsv")) if r.contig == "chr2"}
    checked = 0
    for (b, ga, gb), (row, segs) in facts.items():
        if (ga, gb) != ("fam0.fa", "fam1.fa") or (b, ga) not in starts:
            continue
        sa, sb = starts[(b, ga)], starts[(b, gb)]
        assert row["orientation"] == "+" and row["aligned"] > 1000
        assert all(s[4] == s[2] for s, _ in segs), "a segment off the main diagonal between genomes without indels"
        planted = sum(int((a[sa + s[1]:sa + s[1] + s[2]] != c[sb + s[3]:sb + s[3] + s[4]]).sum()) for s, d in segs if d < B.INVALID)
        print(f"block {b}: {row['edits']} edits, {planted} substitutions inside the aligned stretches")
        assert row["edits"] <= planted
        checked += 1
    assert checked >= 1
    # a block that spans the planted indels: segments with dy != dx that are aligned all the same
    hit = [(s, d) for (b, ga, gb), (row, segs) in facts.items() if gb == "fam2.fa" and row["length_a"] > 250_000 for s, d in segs
           if s[4] != s[2] and d < B.INVALID]
    assert len(hit) >= N_INDELS // 2 and len(indels) == N_INDELS, hit[:3]
    # the inverted block: identity within the family's range (1 % pairwise divergence), far from a random pair's 0.25
    flipped = [row for row, _ in facts.values() if row["orientation"] == "-"]
    assert len(flipped) == 2
    for row in flipped:
        m = max(row["aligned_a"], row["aligned_b"])
        assert m > 10_000 and (m - row["edits"]) / m > 0.98, row

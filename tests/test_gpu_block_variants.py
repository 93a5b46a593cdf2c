"""`ntSynt --block-variants` and `bin/ntsynt_block_stats --variants-out` end to end (ntsynt_amd/assess.py block_variants;
docs/design/04_17_block_variants.md): three genomes of 2 x 60 kbp at 1 % with an 8 kbp inverted stretch in genome 1 -- a block of its
own whose lines differ in strand, which the CPU oracle's table must show -- and four indels of 1 - 12 bases in genome 2, two of them
inside that stretch, each planted where the canonical script keeps it whole (quiet_spot).  The file is recomputed byte for byte on
the CPU (tests/variants_brute.py: the full table and the walk per segment); block_identity.tsv is the same with and without the switch; per pair the ops behind the events number that pair's `edits`;
every planted indel is one event of its length and type in `+` and in `-` pairs; the tool gives the same bytes; without the switch
there is no such file and every other output is what it is with it.  Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, synth
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import variants_brute as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
PARAMS = ["-d", "1", "-k", "24", "-w", "100", "--w_rounds", "50", "10", "--indel", "500", "--merge", "1000", "-b", "2000", "-p", "g"]
ORACLE = dict(prefix="g", k=24, w=100, w_rounds=(50, 10), indel=500, merge=1000, block_size=2000)
K, RATE, BAND, MAX_LEN = 21, 16, 31, 4096                    # the switches' defaults
INVERT_AT, INVERT_BP = 24_000, 8_000                         # genome 1, contig 1; chosen on the CPU: the oracle reports it as a block
# genome 2: (contig, from where in the unedited contig a place is looked for, bases inserted (+) or deleted (-)); the first two lie
# inside the inverted stretch
INDELS = [(0, 26_000, 12), (0, 29_500, -5), (1, 20_000, 1), (1, 40_000, -7)]


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def quiet_spot(contigs, at, n):
    """the first position w >= at where the genomes agree on 15 bases either side of an indel of |n| bases, and where the canonical
    script keeps that indel whole: it takes a match before any edit, so an inserted or deleted base that repeats the base before the
    indel (behind it, in a flipped pair) is matched and the run splits.  Returns (w, the letter to insert)"""
    size = -n if n < 0 else 0
    for w in range(at, at + 5_000):
        lo, hi = w - 15, w + size + 15
        if any((c[lo:hi] != contigs[0][lo:hi]).any() for c in contigs[1:]):
            continue
        flanks = {int(contigs[0][w - 1]), int(contigs[0][w + size])}
        if n > 0:
            return w, [x for x in b"ACGT" if x not in flanks][0]
        if not flanks & set(contigs[0][w:w + size].tolist()):
            return w, None
    raise AssertionError("no such position")


def variants_family(outdir):
    "(paths, genomes, the indels as (contig, position in genome 2's edited contig, bases inserted (+) or deleted (-)))"
    anc = synth.make_ancestor(120_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    planted = []
    for contig in (0, 1):
        c = fam[2][contig]
        pieces, at, size = [], 0, 0
        for _, where, n in [x for x in INDELS if x[0] == contig]:
            where, letter = quiet_spot([g[contig] for g in fam], where, n)
            pieces.append(c[at:where])
            size += where - at
            planted.append((contig, size, n))
            if n > 0:
                pieces.append(np.full(n, letter, dtype=np.uint8))
                size += n
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
    return paths, fam, planted


def recompute(blocks_tsv, fam, names):
    "(variants text, identity text, per pair [ops, event lines]) of tests/variants_brute.py: no GPU, none of assess.block_variants"
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    return V.brute_file(assess.read_blocks(blocks_tsv), genomes, O.hash_all, K, RATE, BAND, MAX_LEN)


def _run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table (checked before any GPU run), four runs -- plain, each switch, both -- and the recomputation"
    tmp = tmp_path_factory.mktemp("block_variants")
    paths, fam, planted = variants_family(str(tmp))
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
    for name, extra in (("plain", []), ("identity", ["--block-identity"]), ("variants", ["--block-variants"]),
                        ("both", ["--block-identity", "--block-variants", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["both"] / "g.synteny_blocks.tsv").read_text() == table
    text, id_text, per_pair = recompute(str(dirs["both"] / "g.synteny_blocks.tsv"), fam, [os.path.basename(p) for p in paths])
    return tmp, paths, fam, planted, dirs, text, id_text, per_pair


def test_the_file_equals_the_recomputation(runs):
    _, _, _, _, dirs, text, _, per_pair = runs
    got = (dirs["both"] / "g.block_variants.tsv").read_text()
    kinds = [ln.split("\t")[8] for ln in text.splitlines()[1:-1]]
    print(f"{len(per_pair)} pairs, {sum(n for n, _ in per_pair.values())} ops, {len(kinds)} events: " + ", ".join(f"{k} {kinds.count(k)}" for k in ("snv", "ins", "del")))
    assert len(kinds) > 3_000 and {"snv", "ins", "del"} == set(kinds)
    assert got == text
    assert (dirs["variants"] / "g.block_variants.tsv").read_text() == text


def test_the_identity_file_is_the_same_with_and_without_the_switch(runs):
    _, _, _, _, dirs, _, id_text, _ = runs
    assert (dirs["identity"] / "g.block_identity.tsv").read_text() == id_text
    assert (dirs["both"] / "g.block_identity.tsv").read_bytes() == (dirs["identity"] / "g.block_identity.tsv").read_bytes()


def test_the_ops_of_a_pair_number_its_edits(runs):
    _, _, _, _, dirs, _, _, per_pair = runs
    lines = (dirs["both"] / "g.block_identity.tsv").read_text().splitlines()
    col = {c: i for i, c in enumerate(lines[0].split("\t"))}
    ops = {}
    for ln in (dirs["both"] / "g.block_variants.tsv").read_text().splitlines()[1:-1]:
        f = ln.split("\t")
        ops[(f[0], f[1], f[4])] = ops.get((f[0], f[1], f[4]), 0) + (1 if f[8] == "snv" else int(f[9]))
    checked = 0
    for ln in lines[1:-1]:
        f = ln.split("\t")
        key = (f[col["block_id"]], f[col["genome_a"]], f[col["genome_b"]])
        assert ops.get(key, 0) == int(f[col["edits"]]) == per_pair[key][0], key
        checked += 1
    assert checked == len(per_pair) >= 12


def test_every_planted_indel_is_one_event(runs):
    _, _, _, planted, dirs, _, _, _ = runs
    events = [ln.split("\t") for ln in (dirs["both"] / "g.block_variants.tsv").read_text().splitlines()[1:-1]]
    seen = {"+": 0, "-": 0}
    for contig, where, n in planted:
        kind, size = ("ins", n) if n > 0 else ("del", -n)
        for name_a in ("fam0.fa", "fam1.fa"):                 # genome 2 is the last of every block's lines: always genome_b
            hits = [e for e in events if e[1] == name_a and e[4] == "fam2.fa" and e[5] == f"chr{contig + 1}" and e[8] == kind and int(e[6]) == where]
            assert len(hits) == 1 and int(hits[0][9]) == size, (contig, where, n, name_a, hits)
            assert (hits[0][10] == "-") == (kind == "ins") and (hits[0][11] == "-") == (kind == "del")
            seen[hits[0][7]] += 1
    assert seen["+"] >= 4 and seen["-"] >= 2, seen


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, _, _, dirs, text, id_text, _ = runs
    out, out_id = tmp / "tool.block_variants.tsv", tmp / "tool.block_identity.tsv"
    fais = [str(dirs["both"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["both"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["both"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--variants-out", str(out), "--identity-out", str(out_id), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text and out_id.read_text() == id_text


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, _, _, dirs, _, _, _ = runs
    same = sorted(os.listdir(dirs["plain"]))
    assert "g.synteny_blocks.tsv" in same and not any("block_variants" in name for name in same)
    for name in same:
        for other in ("identity", "variants", "both"):
            assert (dirs["plain"] / name).read_bytes() == (dirs[other] / name).read_bytes() and (dirs["plain"] / name).stat().st_size > 0, (name, other)
    assert sorted(set(os.listdir(dirs["identity"])) - set(same)) == ["g.block_identity.tsv"]
    assert sorted(set(os.listdir(dirs["variants"])) - set(same)) == ["g.block_variants.tsv"]
    assert sorted(set(os.listdir(dirs["both"])) - set(same)) == ["g.block_identity.tsv", "g.block_variants.tsv", "g.stage_times.tsv"]
    stages = [ln.split("\t")[0] for ln in (dirs["both"] / "g.stage_times.tsv").read_text().splitlines()]
    assert "block_identity" in stages and "block_variants" in stages and stages.index("block_identity") < stages.index("block_variants")

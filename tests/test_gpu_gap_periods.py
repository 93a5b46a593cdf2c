"""`ntSynt --gap-periods` and `bin/ntsynt_gaps --periods-out` end to end (ntsynt_amd/gaps.py periods; docs/design/04_14_gap_periods.md):
a three-genome family of 2 x 300 kbp in which genome 1 alone has (a) an exact array of 40 copies of a 171-base unit and (b) an array of
30 copies of a 340-base unit, each copy with its own 1 % of substitutions, between 5 kbp of random sequence on either side.  (b) is
inserted right behind a segment that genome 1 has on the other strand, which no block covers either: 10 200 bases of array between
2 x 5 000 of flank alone are a hair MORE than half of their gap, with the 6 kbp of the inverted segment in the same gap they are well
under half.  The file is recomputed byte for byte on the CPU -- gaps.cut, O.hash_all of every record, tests/periods_brute.py's
definitions, no filter --; (a)'s gap must read period 171 `tandem` with its extent at the array's ends, (b)'s period 340 `partial`,
the gaps the two other genomes have at the inverted segment `.`; every other file of the run is what it is without the switch; the tool
gives the same bytes.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, gaps, synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.periods_brute import brute_file
from tests.test_gpu_gap_copies import gap_over

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
K, RATE, MIN_HITS = 24, 16, 4                                # -k of L.PARAMS; the switches' defaults
A_AT, A_UNIT, A_COPIES = 90_000, 171, 40                     # genome 1, contig 1: the exact array
INVERT_AT, INVERT_BP = 200_000, 6_000                        # genome 1, contig 1 (coordinates before the insertion): shared, on the other strand
B_AT, B_UNIT, B_COPIES, B_FLANK = INVERT_AT + INVERT_BP, 340, 30, 5_000    # genome 1, contig 1, right behind the inverted segment: random flank, the diverged array, random flank
SEED = 14


def period_family(outdir):
    "(paths, genomes, (start, end) of array a and of array b in genome 1's chr1, as written)"
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(SEED)
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    array_a = np.tile(synth.random_dna(A_UNIT, rng), A_COPIES)
    unit = synth.random_dna(B_UNIT, rng)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    copies = []
    for _ in range(B_COPIES):
        copy = unit.copy()
        for at in rng.choice(B_UNIT, size=round(0.01 * B_UNIT), replace=False):              # its own 1 % of substitutions
            copy[at] = rng.choice(letters[letters != copy[at]])
        copies.append(copy)
    array_b = np.concatenate(copies)
    c = np.concatenate([c[:B_AT], synth.random_dna(B_FLANK, rng), array_b, synth.random_dna(B_FLANK, rng), c[B_AT:]])
    fam[1][0] = np.concatenate([c[:A_AT], array_a, c[A_AT:]])                                  # (a) lies before (b): it moves (b) by its length
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    b_at = B_AT + array_a.size + B_FLANK
    return paths, fam, (A_AT, A_AT + array_a.size), (b_at, b_at + array_b.size)


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def recompute(blocks_tsv, fam, names, k, rate, min_hits):
    "(text of the file, {gap: (sampled, (recurring, period, period_hits, first_off, last_off))}, gaps) from the definitions: no GPU, none of gaps.periods"
    table = assess.read_blocks(blocks_tsv)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, _ = gaps.cut(table, records)
    hashed = {}

    def kmers_of(genome, contig):
        if (genome, contig) not in hashed:
            pos, h0 = O.hash_all(fam[names.index(genome)][int(contig[3:]) - 1].tobytes(), k)
            hashed[(genome, contig)] = (pos.astype(np.int64).tolist(), h0.tolist())
        return hashed[(genome, contig)]
    text, facts = brute_file([(g.genome, g.contig, g.start, g.end, g.kind) for g in cut_gaps], kmers_of, k, rate, min_hits)
    return text, facts, cut_gaps


def fact_of(facts, g):
    return facts[(g.genome, g.contig, g.start, g.end, g.kind)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family with --gap-links --gap-copies, and with --gap-periods beside them"
    tmp = tmp_path_factory.mktemp("gap_periods")
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    (tmp / "fam").mkdir()
    family = period_family(str(tmp / "fam"))
    dirs = {}
    for name, extra in (("without", ["--gap-links", "--gap-copies"]), ("with", ["--gap-links", "--gap-copies", "--gap-periods", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = L._run(ntsynt + family[0] + L.PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, family, dirs


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, dirs = runs
    without, with_it = dirs["without"], dirs["with"]
    same = sorted(os.listdir(without))
    assert {"g.synteny_blocks.tsv", "g.gaps.tsv", "g.gap_summary.tsv", "g.gap_links.tsv", "g.gap_copies.tsv", "g.common.bf"} <= set(same)
    assert "g.gap_periods.tsv" not in same
    for name in same:
        assert (without / name).read_bytes() == (with_it / name).read_bytes() and (without / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_it)) - set(same)) == ["g.gap_periods.tsv", "g.stage_times.tsv"]       # (the latter: --benchmark)
    stages = [ln.split("\t")[0] for ln in (with_it / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_links") < stages.index("gap_copies") < stages.index("gap_periods")


def test_the_file_equals_a_recomputation_and_both_arrays_are_found(runs):
    """The recomputation alone (seed 14, k 24, rate 16) gives for array (a)'s gap and array (b)'s gap the sampled records and the records
    at the period that docs/design/04_14_gap_periods.md quotes; both are printed, and both periods must stand on at least min_hits
    records before the device's file is looked at."""
    _, (paths, fam, span_a, span_b), dirs = runs
    names = [os.path.basename(p) for p in paths]
    out = dirs["with"]
    got = (out / "g.gap_periods.tsv").read_text()
    print(got)
    text, facts, cut_gaps = recompute(str(out / "g.synteny_blocks.tsv"), fam, names, K, RATE, MIN_HITS)
    gap_a = gap_over(cut_gaps, names[1], *span_a)
    gap_b = gap_over(cut_gaps, names[1], *span_b)
    assert gap_b.start <= span_b[0] - B_FLANK * 0.8 and gap_b.end >= span_b[1] + B_FLANK * 0.8, gap_b          # the flanks lie in the same gap
    print("array a:", gap_a, fact_of(facts, gap_a), "array b:", gap_b, fact_of(facts, gap_b))
    assert fact_of(facts, gap_a)[1][2] >= MIN_HITS and fact_of(facts, gap_b)[1][2] >= MIN_HITS                  # the recomputation alone
    assert got.splitlines()[0].split("\t") == list(gaps.PERIOD_COLUMNS)
    assert got == text
    gaps_tsv = (out / "g.gaps.tsv").read_text().splitlines()[1:-1]
    assert [ln.split("\t")[:6] for ln in got.splitlines()[1:-1]] == [ln.split("\t")[:6] for ln in gaps_tsv]     # one line per gap of gaps.tsv, in its order
    rows = {tuple(ln.split("\t")[:4]): dict(zip(gaps.PERIOD_COLUMNS, ln.split("\t"))) for ln in got.splitlines()[1:-1]}
    a = rows[(gap_a.genome, gap_a.contig, str(gap_a.start), str(gap_a.end))]
    assert a["period"] == str(A_UNIT) and a["class"] == "tandem", a
    assert abs(int(a["from"]) - span_a[0]) <= A_UNIT + K and abs(span_a[1] - int(a["to"])) <= A_UNIT + K, (a, span_a)
    b = rows[(gap_b.genome, gap_b.contig, str(gap_b.start), str(gap_b.end))]
    assert b["period"] == str(B_UNIT) and b["class"] == "partial", b
    assert span_b[0] <= int(b["from"]) < int(b["to"]) <= span_b[1], (b, span_b)
    for other in (names[0], names[2]):                                                                          # unique sequence: sampled, nothing recurs
        inv = gap_over(cut_gaps, other, INVERT_AT, INVERT_AT + INVERT_BP)
        i = rows[(inv.genome, inv.contig, str(inv.start), str(inv.end))]
        assert i["class"] == "." and i["period"] == "." and int(i["sampled"]) >= 100, i
    assert sum(r["class"] != "." for r in rows.values()) == 2                                                   # and no other gap has a period


def test_the_tool_reproduces_the_file(runs):
    tmp, (paths, _, _, _), dirs = runs
    out = dirs["with"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf")]
    r = L._run(tool + ["--out", os.devnull, "--summary-out", os.devnull, "--periods-out", str(tmp / "alone.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.tsv").read_bytes() == (out / "g.gap_periods.tsv").read_bytes()
    r = L._run(tool + ["--out", str(tmp / "again.tsv"), "--summary-out", str(tmp / "again_summary.tsv"), "--links-out", str(tmp / "again_links.tsv"),
                       "--copies-out", str(tmp / "again_copies.tsv"), "--periods-out", str(tmp / "again_periods.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    for mine, theirs in (("again_periods.tsv", "g.gap_periods.tsv"), ("again_copies.tsv", "g.gap_copies.tsv"), ("again_links.tsv", "g.gap_links.tsv"),
                         ("again.tsv", "g.gaps.tsv"), ("again_summary.tsv", "g.gap_summary.tsv")):
        assert (tmp / mine).read_bytes() == (out / theirs).read_bytes(), mine

"""`ntSynt --gap-families` and `bin/ntsynt_gaps --families-out / --family-sites-out` end to end (ntsynt_amd/gaps.py families;
docs/design/04_15_gap_families.md): a three-genome family of 2 x 300 kbp in which genome 1 alone has an exact array of 40 copies of a
171-base unit S1, a second S1 array of 25 copies elsewhere, each copy with its own 1 % of substitutions, and an array of 30 copies of an
unrelated 340-base unit S2; genome 2 alone has an S1 array of 15 copies at a place of its own; and all three genomes carry 8 copies of
S1 at one orthologous place inside otherwise collinear sequence.  Both files are recomputed byte for byte on the CPU -- gaps.cut,
O.hash_all of every record, the definitions of tests/periods_brute.py and tests/families_brute.py, no filter, no set --; the S1 arrays
of the two genomes must be one family, S2 a family of its own, some S1 site must lie inside a block and some gap must be no array;
every other file of the run is what it is with --gap-periods only; the tool gives the same bytes.  Every test runs under a time limit
of its own."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, gaps, synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.families_brute import brute_files
from tests.periods_brute import brute_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
K, RATE, MIN_HITS, STEP = 24, 16, 4, 1000                    # -k of L.PARAMS; the switches' defaults
S1_UNIT, S2_UNIT = 171, 340
# genome 1, contig 1 (coordinates before any insertion): the exact S1 array, the diverged S1 array, a shared segment on the other strand,
# the S2 array
A_AT, A_COPIES = 90_000, 40
D_AT, D_COPIES = 150_000, 25
INVERT_AT, INVERT_BP = 200_000, 6_000
B_AT, B_COPIES = 250_000, 30
C_AT, C_COPIES = 60_000, 15                                  # genome 2, contig 1: an S1 array of its own
O_AT, O_COPIES = 150_000, 8                                  # every genome, contig 2: S1 at one orthologous place
SEED = 15


def families_family(outdir):
    """(paths, genomes, spans): spans = {name: (genome index, contig index, start, end) as written} of the five arrays and of the
    orthologous copies in each genome (`ortho0`, `ortho1`, `ortho2`)"""
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(SEED)
    s1, s2 = synth.random_dna(S1_UNIT, rng), synth.random_dna(S2_UNIT, rng)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    copies = []
    for _ in range(D_COPIES):
        copy = s1.copy()
        for at in rng.choice(S1_UNIT, size=round(0.01 * S1_UNIT), replace=False):            # its own 1 % of substitutions
            copy[at] = rng.choice(letters[letters != copy[at]])
        copies.append(copy)
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    spans, moved = {}, 0
    pieces, at = [], 0
    for name, where, array in (("s1_exact", A_AT, np.tile(s1, A_COPIES)), ("s1_diverged", D_AT, np.concatenate(copies)), ("s2", B_AT, np.tile(s2, B_COPIES))):
        pieces += [c[at:where], array]
        spans[name] = (1, 0, where + moved, where + moved + array.size)
        moved += array.size
        at = where
    fam[1][0] = np.concatenate(pieces + [c[at:]])
    own = np.tile(s1, C_COPIES)
    fam[2][0] = np.concatenate([fam[2][0][:C_AT], own, fam[2][0][C_AT:]])
    spans["s1_own"] = (2, 0, C_AT, C_AT + own.size)
    shared = np.tile(s1, O_COPIES)
    for j in range(3):
        fam[j][1] = np.concatenate([fam[j][1][:O_AT], shared, fam[j][1][O_AT:]])
        spans[f"ortho{j}"] = (j, 1, O_AT, O_AT + shared.size)
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam, spans


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def recompute(blocks_tsv, fam, names, k=K, rate=RATE, min_hits=MIN_HITS, step=STEP):
    """(periods text, families text, sites text, facts, gaps) from the definitions: no GPU, none of gaps.periods or gaps.families"""
    table = assess.read_blocks(blocks_tsv)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, _ = gaps.cut(table, records)
    hashed = {}

    def kmers_of(genome, contig):
        if (genome, contig) not in hashed:
            pos, h0 = O.hash_all(fam[names.index(genome)][int(contig[3:]) - 1].tobytes(), k)
            hashed[(genome, contig)] = (pos.astype(np.int64).tolist(), h0.tolist())
        return hashed[(genome, contig)]
    as_tuples = [(g.genome, g.contig, g.start, g.end, g.kind) for g in cut_gaps]
    periods_text, _ = brute_file(as_tuples, kmers_of, k, rate, min_hits)
    period_lines = [ln.split("\t") for ln in periods_text.splitlines()[1:-1]]
    families_text, sites_text, facts = brute_files(as_tuples, period_lines, kmers_of, {name: [c for c, _ in records[name]] for name in names}, table,
                                                   k, rate, min_hits, step)
    return periods_text, families_text, sites_text, facts, as_tuples


def named_facts(facts, as_tuples, names, spans):
    """the facts the family is built to show, from a recomputation alone: (family of S1, family of S2).  At least two families; the S1
    family has member arrays in two genomes; S2 is a family of its own; some S1 site lies inside a block; some gap is no array."""
    def array_over(name):
        j, contig, a, b = spans[name]
        found = [i for i, g in enumerate(facts["arrays"]) if g[0] == names[j] and g[1] == f"chr{contig + 1}" and g[2] < b and g[3] > a]
        assert len(found) == 1, (name, found)
        return found[0]
    families = facts["family_of_array"]
    s1 = families[array_over("s1_exact")]
    assert families[array_over("s1_diverged")] == s1 and families[array_over("s1_own")] == s1, families
    s2 = families[array_over("s2")]
    assert s2 != s1 and families.count(s2) == 1 and len(set(families)) >= 2, families
    assert {facts["arrays"][i][0] for i, f in enumerate(families) if f == s1} >= {names[1], names[2]}
    in_blocks = [s for s in facts["sites"] if s[0] == s1 and s[6] == "block"]
    assert in_blocks, facts["sites"]
    for j in range(3):                                           # the orthologous copies are found in every genome
        _, contig, a, b = spans[f"ortho{j}"]
        assert any(s[0] == s1 and s[1] == names[j] and s[2] == f"chr{contig + 1}" and s[3] < b and s[4] > a for s in facts["sites"]), (j, facts["sites"])
    assert len(as_tuples) > len(families)                        # a gap that is no array
    assert not any(s[0] == s2 and s[1] != names[1] for s in facts["sites"])                    # S2 is genome 1's alone
    return s1, s2


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family with --gap-links --gap-periods, and with --gap-families beside them"
    tmp = tmp_path_factory.mktemp("gap_families")
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    (tmp / "fam").mkdir()
    family = families_family(str(tmp / "fam"))
    dirs = {}
    for name, extra in (("without", ["--gap-links", "--gap-periods"]), ("with", ["--gap-links", "--gap-families", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = L._run(ntsynt + family[0] + L.PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, family, dirs


def test_the_switch_adds_two_files_and_changes_none(runs):
    _, _, dirs = runs
    without, with_it = dirs["without"], dirs["with"]
    same = sorted(os.listdir(without))
    assert {"g.synteny_blocks.tsv", "g.gaps.tsv", "g.gap_summary.tsv", "g.gap_links.tsv", "g.gap_periods.tsv", "g.common.bf"} <= set(same)
    assert "g.gap_families.tsv" not in same and "g.gap_family_sites.tsv" not in same
    for name in same:
        assert (without / name).read_bytes() == (with_it / name).read_bytes() and (without / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_it)) - set(same)) == ["g.gap_families.tsv", "g.gap_family_sites.tsv", "g.stage_times.tsv"]   # (the last: --benchmark)
    stages = [ln.split("\t")[0] for ln in (with_it / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_links") < stages.index("gap_periods") < stages.index("gap_families")


def test_both_files_equal_a_recomputation_and_the_families_are_found(runs):
    """The recomputation alone (seed 15, k 24, rate 16, min_hits 4, step 1000) must show the named facts before the device's files are
    looked at: docs/design/04_15_gap_families.md quotes its lines."""
    _, (paths, fam, spans), dirs = runs
    names = [os.path.basename(p) for p in paths]
    out = dirs["with"]
    got_f, got_s = (out / "g.gap_families.tsv").read_text(), (out / "g.gap_family_sites.tsv").read_text()
    print(got_f)
    print(got_s)
    periods_text, families_text, sites_text, facts, as_tuples = recompute(str(out / "g.synteny_blocks.tsv"), fam, names)
    s1, s2 = named_facts(facts, as_tuples, names, spans)                                        # the recomputation alone
    print("S1 is family", s1, "S2 is family", s2)
    assert (out / "g.gap_periods.tsv").read_text() == periods_text
    assert got_f.splitlines()[0].split("\t") == list(gaps.FAMILY_COLUMNS) and got_s.splitlines()[0].split("\t") == list(gaps.FAMILY_SITE_COLUMNS)
    assert got_f == families_text
    assert got_s == sites_text
    rows = [dict(zip(gaps.FAMILY_COLUMNS, ln.split("\t"))) for ln in got_f.splitlines()[1:-1]]
    mine = [r for r in rows if r["family"] == str(s1)]
    assert {r["genome"] for r in mine} == {names[1], names[2]} and all(r["members"] == str(len(mine)) and r["genomes"] == "2" for r in mine), mine
    assert all(r["period"] == str(S1_UNIT) and int(r["shared_hashes"]) >= 1 for r in mine), mine
    other = [r for r in rows if r["family"] == str(s2)]
    assert len(other) == 1 and (other[0]["genome"], other[0]["period"], other[0]["members"], other[0]["genomes"], other[0]["shared_hashes"]) == \
        (names[1], str(S2_UNIT), "1", "1", "0"), other
    sites = [dict(zip(gaps.FAMILY_SITE_COLUMNS, ln.split("\t"))) for ln in got_s.splitlines()[1:-1]]
    assert [(int(s["family"]), s["genome"]) for s in sites] == sorted((int(s["family"]), s["genome"]) for s in sites)
    assert {s["placement"] for s in sites if s["family"] == str(s1)} >= {"array", "block"}
    assert got_f.splitlines()[-1] == got_s.splitlines()[-1] and got_f.splitlines()[-1].startswith(f"# k {K}, rate {RATE}, min_hits {MIN_HITS}, step {STEP}, arrays {len(rows)}, families ")


def test_the_tool_reproduces_both_files(runs):
    tmp, (paths, _, _), dirs = runs
    out = dirs["with"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf"), "--out", os.devnull, "--summary-out", os.devnull]
    r = L._run(tool + ["--families-out", str(tmp / "alone_f.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone_f.tsv").read_bytes() == (out / "g.gap_families.tsv").read_bytes()
    r = L._run(tool + ["--family-sites-out", str(tmp / "alone_s.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone_s.tsv").read_bytes() == (out / "g.gap_family_sites.tsv").read_bytes()
    r = L._run(tool + ["--links-out", str(tmp / "again_links.tsv"), "--periods-out", str(tmp / "again_periods.tsv"), "--families-out", str(tmp / "again_f.tsv"),
                       "--family-sites-out", str(tmp / "again_s.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    for mine, theirs in (("again_f.tsv", "g.gap_families.tsv"), ("again_s.tsv", "g.gap_family_sites.tsv"), ("again_periods.tsv", "g.gap_periods.tsv"),
                         ("again_links.tsv", "g.gap_links.tsv")):
        assert (tmp / mine).read_bytes() == (out / theirs).read_bytes(), mine

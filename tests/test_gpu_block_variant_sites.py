"""`ntSynt --block-variant-sites` and `bin/ntsynt_block_stats --variant-sites-out` end to end (ntsynt_amd/assess.py block_variant_sites;
docs/design/04_32_block_variant_sites.md) on the family of tests/test_gpu_block_paf.py -- three genomes of 120 kbp with the planted
indels -- with --identity-max-edits 1023 --block-ends, and again with E = 0 and no ends, each run with --block-paf --paf-cs
--block-conservation --block-variant-sites.  The file is recomputed without the GPU from the run's PAF alone: the cg:Z: CIGARs of the
star pairs' records give the entries and their cs:Z: texts the bases, both trimmed to the cores, and tests/variant_sites_brute.py walks
them column by column.  Every test runs under a time limit of its own."""
import faulthandler
import os
import re
import sys

import pytest

from ntsynt_amd import assess
from tests import variant_sites_brute as VB
from tests.test_gpu_block_end_variants import PARAMS
from tests.test_gpu_block_paf import BAND, ENDS_MAX_EDITS, ENDS_MAX_LEN, ENDS_PENALTY, K, MAX_EDITS, MAX_LEN, RATE, ROOT, SWITCHES, _run, paf_family

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
NTSYNT = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
PAF, BED, SITES = "g.block_alignments.paf", "g.block_conservation.bed", "g.block_variant_sites.tsv"
WIDE = ["--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN)]
OTHERS = ["--block-paf", "--paf-cs", "--block-conservation"]
TIMERS = ["cigar_var_bases_scan", "cigar_var_bases_emit", "cigar_alleles_events", "cigar_alleles_emit"]
CODES = {"I": VB.I, "D": VB.D, "=": VB.EQ, "X": VB.X}
PARAMETERS = {"full": (K, RATE, BAND, MAX_LEN, MAX_EDITS, (ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY)), "narrow": (K, RATE, BAND, MAX_LEN, 0, None)}


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and its runs: E = 1023 with ends without the switch and with it; E = 0 without ends with it"
    tmp = tmp_path_factory.mktemp("variant_site_runs")
    paths, _ = paf_family(str(tmp))
    dirs = {}
    for key, switches in (("without", SWITCHES + OTHERS), ("full", SWITCHES + OTHERS + ["--block-variant-sites"]), ("narrow", OTHERS + ["--block-variant-sites"])):
        dirs[key] = tmp / ("run_" + key)
        dirs[key].mkdir()
        r = _run(NTSYNT + paths + PARAMS + switches, dirs[key])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, dirs


def star_cores(run_dir):
    """(groups, chains, chain_row, alts, ref, alt) for tests/variant_sites_brute.py from the run's block table and PAF alone: the star
    pairs' CIGARs trimmed to their cores, the bases of their X, D and I entries from the cs:Z: texts, the chains by (block, row, t0)"""
    table = assess.read_blocks(str(run_dir / "g.synteny_blocks.tsv"))
    lines_of = {}
    for r in table:
        lines_of.setdefault(r.block_id, []).append(r)
    order = sorted(lines_of, key=lambda b: (0, int(b), "") if b.lstrip("-").isdigit() else (1, 0, b))
    groups = [(b, lines_of[b][0].genome, lines_of[b][0].contig, lines_of[b][0].start, lines_of[b][0].end, len(lines_of[b]) - 1) for b in order]
    held = []
    for line in (run_dir / PAF).read_text().splitlines():
        f = line.split("\t")
        block, tg, qg, cg, cs = f[13][5:], f[14][5:], f[15][5:], f[17][5:], f[18][5:]
        assert f[18].startswith("cs:Z:") and f[17].startswith("cg:Z:")
        lines = lines_of[block]
        if tg != lines[0].genome:
            continue                                          # (no star pair)
        entries = [int(n) << 4 | CODES[c] for n, c in re.findall(r"(\d+)([ID=X])", cg)]
        tokens = re.findall(r":\d+|\*[a-z]{2}|\+[a-z]+|-[a-z]+", cs)
        assert "".join(tokens) == cs
        bases, at = [], 0                                     # per entry (its ref bytes, its alt bytes)
        for v in entries:
            code, size = v & 15, v >> 4
            if code == VB.X:
                mine = tokens[at:at + size]
                assert all(t[0] == "*" for t in mine) and len(mine) == size
                bases.append(("".join(t[1] for t in mine).upper(), "".join(t[2] for t in mine).upper()))
                at += size
            else:
                t = tokens[at]
                at += 1
                assert t[0] == {VB.EQ: ":", VB.I: "+", VB.D: "-"}[code] and (int(t[1:]) if code == VB.EQ else len(t) - 1) == size, (t, v)
                bases.append(("", "") if code == VB.EQ else ("", t[1:].upper()) if code == VB.I else (t[1:].upper(), ""))
        assert at == len(tokens)
        both = [i for i, v in enumerate(entries) if v & 15 in (VB.EQ, VB.X)]
        if not both:
            continue
        t0 = int(f[7]) + sum(v >> 4 for v in entries[:both[0]] if v & 15 == VB.D)
        core = slice(both[0], both[-1] + 1)
        row = [ln.genome for ln in lines].index(qg)
        held.append((order.index(block), row, t0, entries[core], "".join(b[0] for b in bases[core]), "".join(b[1] for b in bases[core])))
    held.sort(key=lambda h: h[:3])
    chains = [(h[0], h[2], h[3]) for h in held]
    return (groups, chains, [h[1] for h in held], [h[5].encode() for h in held], "".join(h[4] for h in held).encode(), "".join(h[5] for h in held).encode())


def brute_text(run_dir, key):
    groups, chains, chain_row, alts, ref, alt = star_cores(run_dir)
    found, _, carriers = VB.alleles(chains, alts, len(groups))
    types = VB.genotypes(found, carriers, chains, chain_row, [g[5] for g in groups])
    return VB.table_text(groups, found, ref, alt, types, PARAMETERS[key]), found, types


def test_the_file_equals_the_brute_force_text(runs):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        want, found, types = brute_text(dirs[key], key)
        print(key, len(found), "alleles;", sum(1 for a in found if a[7] > 1), "with two carriers;", sum(1 for t in types if "." in t), "lines with a `.`;",
              {k: sum(1 for a in found if a[6] == k) for k in (1, 2, 3)})
        assert {a[6] for a in found} == {VB.SNV, VB.DEL, VB.INS} and len(found) > 100
        assert any(a[7] == 2 for a in found), "an allele that both other genomes carry"
        assert any("." in t for t in types), "an allele at which one of the other genomes is not aligned"
        got = (dirs[key] / SITES).read_text()
        assert got.count("\n") == want.count("\n"), (key, got.count("\n"), want.count("\n"))
        assert got == want, (key, [(g, w) for g, w in zip(got.splitlines(), want.splitlines()) if g != w][:2])
    assert (dirs["narrow"] / SITES).read_bytes() != (dirs["full"] / SITES).read_bytes()


def test_the_snv_carriers_sum_to_the_mismatches_of_the_conservation_bed(runs):
    _, _, dirs = runs
    for key in ("full", "narrow"):
        lines = (dirs[key] / SITES).read_text().splitlines()
        assert lines[0].split("\t") == list(assess.VARIANT_SITES_COLUMNS) and lines[-1].startswith("# k ")
        rows = [ln.split("\t") for ln in lines[1:-1]]
        snv = sum(int(f[10]) for f in rows if f[4] == "snv")
        bed = [ln.split("\t") for ln in (dirs[key] / BED).read_text().splitlines() if not ln.startswith("#")]
        mismatches = sum((int(f[6]) - int(f[7]) - int(f[9])) * (int(f[2]) - int(f[1])) for f in bed)
        assert snv == mismatches > 100, (key, snv, mismatches)
        deleted = sum(int(f[10]) * int(f[5]) for f in rows if f[4] == "del")
        assert deleted == sum(int(f[9]) * (int(f[2]) - int(f[1])) for f in bed), key      # (and the deleted bases to its gap counts)
        for f in rows:
            assert len(f[11]) == int(f[8]) and f[11].count("1") == int(f[10]) and len(f[11]) - f[11].count(".") == int(f[9]) and set(f[11]) <= set("01."), f
            assert (f[6] == "-") == (f[4] == "ins") and (f[7] == "-") == (f[4] == "del") and set(f[6] + f[7]) <= set("ACGTN-"), f


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs = runs
    same = sorted(os.listdir(dirs["without"]))
    assert PAF in same and BED in same and SITES not in same
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == [SITES]
    stages = {key: [ln.split("\t")[0] for ln in (dirs[key] / "g.stage_times.tsv").read_text().splitlines()] for key in ("without", "full")}
    assert [s for s in stages["full"] if s.startswith("block_variant_sites")] == ["block_variant_sites"] + ["block_variant_sites:" + t for t in TIMERS]
    assert stages["full"].index("block_variant_sites") > stages["full"].index("block_conservation")
    assert [s for s in stages["full"] if not s.startswith("block_variant_sites")] == stages["without"]
    assert not any("cigar_var_bases" in s or "cigar_alleles" in s for s in stages["without"])


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs = runs
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais + ["--fastas"] + paths
    r = _run(tool + ["--variant-sites-out", str(tmp / "tool.sites.tsv"), "--identity-max-edits", str(MAX_EDITS), "--ends-out", str(tmp / "tool.ends.tsv"),
                     "--ends-max-len", str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "tool.sites.tsv").read_bytes() == (dirs["full"] / SITES).read_bytes()
    r = _run(tool + ["--variant-sites-out", str(tmp / "alone.sites.tsv"), "--divergence-out", str(tmp / "tool.div2.tsv")], tmp)        # E = 0, no ends
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.sites.tsv").read_bytes() == (dirs["narrow"] / SITES).read_bytes()


def test_dry_run_lists_the_stage_and_several_ranks_are_refused(runs):
    tmp, paths, _ = runs
    r = _run(NTSYNT + paths + PARAMS + WIDE + ["--block-variant-sites", "--dry-run"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    listed = [ln for ln in (r.stdout + r.stderr).splitlines() if "block_variant_sites (" in ln]
    assert len(listed) == 1 and "block_variant_sites (" + ", ".join(TIMERS) + "; k " in listed[0] and f"max_edits {MAX_EDITS}" in listed[0] and \
        f"ends_max_len {ENDS_MAX_LEN}" in listed[0], listed
    r = _run(NTSYNT + paths + PARAMS + ["--block-variant-sites"], tmp, WORLD_SIZE="2", RANK="0")
    assert r.returncode == 2 and "--block-variant-sites works from the genomes resident on one GPU" in r.stderr and "--variant-sites-out" in r.stderr, \
        r.stderr[-2000:]

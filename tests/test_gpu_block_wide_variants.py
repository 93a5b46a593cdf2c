"""`ntSynt --block-wide-variants --identity-max-edits E` and `bin/ntsynt_block_stats --wide-variants-out ... --identity-max-edits E`
end to end (ntsynt_amd/assess.py block_wide_variants; docs/design/04_19_block_wide_variants.md) on the family of
tests/test_gpu_block_identity_wide.py: three genomes of 2 x 60 kbp at 1 %, an 8 kbp inverted stretch in genome 1, and in genome 2
indels of 40, 150, 400 and 900 bases.  On the CPU first (tests/wide_variants_brute.py on the oracle's hashes).  Then the runs: the file
equals the recomputation byte for byte, in `+` and `-` pairs; the planted 40-, 150- and 400-base indels are there as inserted or
deleted bases of one stretch; per pair the ops number the pair's `edits` under E; the tool reproduces the file; with --block-identity
the identity file is the wide pass's; without the new switch every other file is the plain run's.  Every test runs under a time limit
of its own."""
import faulthandler
import os
import sys

import pytest

from ntsynt_amd import assess
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import identity_brute as B
from tests import wide_variants_brute as WV
from tests.test_gpu_block_identity_wide import BAND, K, MAX_EDITS, MAX_LEN, ORACLE, PARAMS, RATE, ROOT, _run, rows_of, wide_family

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
FOOTER = f"# k {K}, rate {RATE}, band {BAND}, max_len {MAX_LEN}, max_edits {MAX_EDITS}"


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


PLANTED = {40, 150, 400}                                     # (the 900-base deletion splits its block: it lies between blocks)


def planted_stretches(per_pair):
    "(pair, kind of event, length difference, inserted or deleted bases, first and last pos_a) of every offband stretch with a planted length"
    out = []
    for key, (_, _, stretches) in per_pair.items():
        for seg, _, n_ins, n_del, a_lo, a_hi in stretches:
            gap = abs(seg[4] - seg[2])
            if seg[5] == B.OFFBAND and gap in PLANTED:
                out.append((key, "ins", gap, n_ins, a_lo, a_hi) if seg[4] > seg[2] else (key, "del", gap, n_del, a_lo, a_hi))
    return out


def bases_in_stretch(rows, key, kind, a_lo, a_hi):
    "the summed `length` of the events of `kind` of one pair that lie inside one stretch (rows: the file's lines, split)"
    return sum(int(f[9]) for f in rows if (f[0], f[1], f[4]) == key and f[8] == kind and a_lo <= int(f[3]) <= a_hi)


def check_stretches(lines, per_pair):
    """every planted indel, as the inserted or deleted bases of its own stretch: rule 1 may move or split the indel, so the assertion is
    on the stretch's total, which is at least the length difference and exactly what the brute script of that stretch holds"""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    seen = {}
    for key, kind, gap, n_bases, a_lo, a_hi in planted_stretches(per_pair):
        got = bases_in_stretch(rows, key, kind, a_lo, a_hi)
        assert got == n_bases and got >= gap, (key, kind, gap, n_bases, got)
        seen.setdefault(gap, set()).add(next(f[7] for f in rows if (f[0], f[1], f[4]) == key))
    return seen


def check_on_the_cpu(text, id_text, per_pair):
    "what the recomputation must show before any GPU run is looked at; returns {planted length: orientations of the pairs that hold it}"
    lines = text.splitlines()
    assert lines[0].split("\t") == list(assess.VARIANT_COLUMNS) and lines[-1] == FOOTER
    identity = rows_of(id_text)
    assert identity.keys() == per_pair.keys()
    for key, (n_ops, _, _) in per_pair.items():
        assert n_ops == int(identity[key]["edits"]), key
    seen = check_stretches(lines, per_pair)
    print("planted indels found whole between two anchors:", {g: sorted(o) for g, o in seen.items()})
    assert set(seen) == PLANTED, (seen, "a planted indel of 40, 150 or 400 bases does not lie whole between two anchors of a block")
    assert {identity[key]["orientation"] for key in per_pair} == {"+", "-"}
    assert any("-" in o for o in seen.values()), "no planted indel in a pair of differing strands"
    return seen


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table, the recomputation (checked before any GPU run) and the runs"
    tmp = tmp_path_factory.mktemp("block_wide_variants")
    paths, fam = wide_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    (tmp / "oracle" / "table.tsv").write_text(table)
    genomes = {os.path.basename(p): {f"chr{i + 1}": c for i, c in enumerate(contigs)} for p, contigs in zip(paths, fam)}
    text, id_text, per_pair = WV.brute_file(assess.read_blocks(str(tmp / "oracle" / "table.tsv")), genomes, O.hash_all, K, RATE, BAND, MAX_LEN, MAX_EDITS)
    check_on_the_cpu(text, id_text, per_pair)
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    e = ["--identity-max-edits", str(MAX_EDITS)]
    dirs = {}
    for name, extra in (("plain", []), ("identity", ["--block-identity"] + e), ("alone", ["--block-wide-variants"] + e),
                        ("both", ["--block-wide-variants", "--block-identity", "--benchmark"] + e)):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["alone"] / "g.synteny_blocks.tsv").read_text() == table
    return tmp, paths, dirs, text, id_text, per_pair


def test_the_file_equals_the_recomputation(runs):
    _, _, dirs, text, _, _ = runs
    got = (dirs["alone"] / "g.block_wide_variants.tsv").read_text()
    assert got.splitlines()[-1] == FOOTER
    assert got == text
    assert (dirs["both"] / "g.block_wide_variants.tsv").read_text() == text
    orientations = {ln.split("\t")[7] for ln in got.splitlines()[1:-1]}
    assert orientations == {"+", "-"}


def test_the_planted_indels_appear_as_ins_or_del_events(runs):
    "each of the 40-, 150- and 400-base indels: the inserted or deleted bases of its stretch, counted inside that stretch alone"
    _, _, dirs, _, _, per_pair = runs
    for name in ("alone", "both"):
        found = check_stretches((dirs[name] / "g.block_wide_variants.tsv").read_text().splitlines(), per_pair)
        assert set(found) == PLANTED, found
        assert any("-" in o for o in found.values())


def test_the_ops_of_a_pair_number_its_edits_under_e(runs):
    _, _, dirs, _, id_text, per_pair = runs
    identity = rows_of((dirs["both"] / "g.block_identity.tsv").read_text())
    bases = {}
    for ln in (dirs["both"] / "g.block_wide_variants.tsv").read_text().splitlines()[1:-1]:
        f = ln.split("\t")
        bases[(f[0], f[1], f[4])] = bases.get((f[0], f[1], f[4]), 0) + int(f[9])        # (an event of `length` bases is that many ops)
    for key, row in identity.items():
        assert bases.get(key, 0) == int(row["edits"]) == per_pair[key][0], key
    assert any(int(r["edits"]) > 0 for r in identity.values())


def test_with_block_identity_the_identity_file_is_the_wide_pass_s(runs):
    _, _, dirs, _, id_text, _ = runs
    assert (dirs["both"] / "g.block_identity.tsv").read_text() == id_text == (dirs["identity"] / "g.block_identity.tsv").read_text()
    assert not (dirs["alone"] / "g.block_identity.tsv").exists()
    stages = [ln.split("\t")[0] for ln in (dirs["both"] / "g.stage_times.tsv").read_text().splitlines()]
    for name in ("block_wide_variants", "block_wide_variants:edit_wide_script_plan", "block_wide_variants:edit_wide_script", "block_identity:edit_wide"):
        assert name in stages, (name, stages)


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs, text, id_text, _ = runs
    out, out_id = tmp / "tool.block_wide_variants.tsv", tmp / "tool.block_identity.tsv"
    fais = [str(dirs["alone"] / (os.path.basename(p) + ".fai")) for p in paths]
    assert all(os.path.exists(f) for f in fais), os.listdir(dirs["alone"])
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["alone"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--wide-variants-out", str(out), "--identity-out", str(out_id), "--identity-max-edits", str(MAX_EDITS),
                                     "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_text() == text and out_id.read_text() == id_text


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, dirs, _, _, _ = runs
    same = sorted(os.listdir(dirs["plain"]))
    assert "g.synteny_blocks.tsv" in same
    for name in same:
        assert (dirs["plain"] / name).read_bytes() == (dirs["alone"] / name).read_bytes() == (dirs["both"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["alone"])) - set(same)) == ["g.block_wide_variants.tsv"]
    assert sorted(set(os.listdir(dirs["both"])) - set(same)) == ["g.block_identity.tsv", "g.block_wide_variants.tsv", "g.stage_times.tsv"]
    assert sorted(set(os.listdir(dirs["identity"])) - set(same)) == ["g.block_identity.tsv"]

"""`ntSynt --gap-copies` and `bin/ntsynt_gaps --copies-out` end to end (ntsynt_amd/gaps.py copies; docs/design/04_12_gap_copies.md): on
tests/test_gpu_gap_block_links.py's family (a 6 kbp copy of genome 1's chr2 inserted into its chr1) and tests/test_gpu_gap_links.py's
(an inverted segment, a private insertion) the file is recomputed byte for byte on the CPU -- gaps.cut, O.hash_all of every record, the
run's filter file, the definitions -- and the copy's gap must read `repeat`, the inversion's gaps `unique`; the tool gives the same
bytes; a run without the switch is what it was.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, gaps
from oracle import nts_oracle as O
from tests import test_gpu_gap_block_links as B
from tests import test_gpu_gap_links as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
U64_MAX = (1 << 64) - 1
RATE = 16                                                   # --gap-links-rate's default
HEADER = ("genome contig start end left_block right_block sampled single_own single_all absent_some copies_own_median copies_own_max "
          "copies_any_median class").split()


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def recompute(blocks_tsv, common_bf, fam, names, rate):
    "(text of the file, rows, gaps, absent, sampled) from gaps.cut, the oracle's hashes, the filter file and the definitions: no GPU, none of gaps.copies"
    from ntsynt_amd.pipeline import read_bf
    bits, k = read_bf(common_bf)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, _ = gaps.cut(assess.read_blocks(blocks_tsv), records)
    thresh = np.uint64(U64_MAX // rate)
    order = sorted(names)
    low, times = {}, {}                                                         # genome -> contig -> (positions, hashes) under the threshold; genome -> {hash: occurrences}
    for name in order:
        low[name] = {}
        for i, c in enumerate(fam[names.index(name)]):
            pos, h0 = O.hash_all(c.tobytes(), k)
            keep = h0 <= thresh
            low[name][f"chr{i + 1}"] = (pos[keep].astype(np.int64), h0[keep])
        keys, mult = np.unique(np.concatenate([h for _, h in low[name].values()]), return_counts=True)
        times[name] = dict(zip((int(x) for x in keys), (int(x) for x in mult)))
    held = {name: {contig: np.array([O.bf_contains(bits, h) for h in h0], dtype=bool) for contig, (_, h0) in low[name].items()} for name in order}
    sampled_hashes = set()
    rows, absent, total = [], 0, 0
    for g in cut_gaps:                                                          # gaps.tsv's order: genome by name, records in file order, by start
        pos, h0 = low[g.genome][g.contig]
        mine = [int(h) for h in h0[(pos >= g.start) & (pos + k <= g.end) & held[g.genome][g.contig]]]
        sampled_hashes.update(mine)
        m = len(mine)
        lead = [g.genome, g.contig, g.start, g.end, g.left_block, g.right_block]
        if m == 0:
            rows.append(lead + [0, 0, 0, "NA", "NA", "NA", "NA", "."])
            continue
        own = [times[g.genome].get(h, 0) for h in mine]
        every = [[times[t].get(h, 0) for t in order] for h in mine]
        single_own, single_all = sum(c == 1 for c in own), sum(all(c == 1 for c in cs) for cs in every)
        absent_some = sum(any(c == 0 for c in cs) for cs in every)
        kind = "unique" if 2 * single_all > m else "repeat" if 2 * (m - single_own) > m else "mixed"
        rows.append(lead + [m, single_own, single_all, absent_some, sorted(own)[(m - 1) // 2], max(own), sorted(max(cs) for cs in every)[(m - 1) // 2], kind])
        absent += absent_some
        total += m
    text = "".join("\t".join(str(v) for v in r) + "\n" for r in [HEADER] + rows)
    footer = f"# k {k}, rate {rate}, filter {bits.size * 8} bits, set {len(sampled_hashes)} hashes, absent {absent} of {total} sampled\n"
    return text + footer, rows, cut_gaps, absent, total


def gap_over(cut_gaps, genome, a, b):
    "the gap of chr1 of `genome` that holds [a, b): the segment lies in ONE gap, not in a block"
    best = max((g for g in cut_gaps if g.genome == genome and g.contig == "chr1"), key=lambda g: min(g.end, b) - max(g.start, a))
    assert min(best.end, b) - max(best.start, a) >= (b - a) * 0.8, (genome, a, b, best)
    return best


def row_of(rows, gap):
    mine = [r for r in rows if (r[0], r[1], r[2], r[3]) == (gap.genome, gap.contig, gap.start, gap.end)]
    assert len(mine) == 1
    return dict(zip(HEADER, mine[0]))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the copy family with --gap-block-links and with --gap-copies beside it; the inversion family with --gap-copies alone"
    tmp = tmp_path_factory.mktemp("gap_copies")
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    families, dirs = {}, {}
    for fam_name, build in (("copy", B.copy_family), ("inv", L.gap_family)):
        (tmp / fam_name).mkdir()
        families[fam_name] = build(str(tmp / fam_name))
    for name, fam_name, extra in (("block_links", "copy", ["--gap-block-links"]), ("all", "copy", ["--gap-block-links", "--gap-copies", "--benchmark"]),
                                  ("alone", "inv", ["--gap-copies"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = L._run(ntsynt + families[fam_name][0] + L.PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, families, dirs


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, dirs = runs
    without, with_all, alone = dirs["block_links"], dirs["all"], dirs["alone"]
    same = sorted(os.listdir(without))
    assert "g.synteny_blocks.tsv" in same and "g.gap_block_links.tsv" in same and "g.gap_copies.tsv" not in same
    for name in same:
        assert (without / name).read_bytes() == (with_all / name).read_bytes() and (without / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_all)) - set(same)) == ["g.gap_copies.tsv", "g.stage_times.tsv"]       # (the latter: --benchmark)
    stages = [ln.split("\t")[0] for ln in (with_all / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_links") < stages.index("gap_block_links") < stages.index("gap_copies")
    listing = set(os.listdir(alone))                                            # the switch alone: the two gap files and its own, neither link file
    assert {"g.gaps.tsv", "g.gap_summary.tsv", "g.gap_copies.tsv"} <= listing and not {"g.gap_links.tsv", "g.gap_block_links.tsv", "g.stage_times.tsv"} & listing


def test_the_copy_family_file_equals_a_recomputation_and_the_copy_is_a_repeat(runs):
    _, families, dirs = runs
    paths, fam = families["copy"]
    names = [os.path.basename(p) for p in paths]
    out = dirs["all"]
    got = (out / "g.gap_copies.tsv").read_text()
    print(got)
    text, rows, cut_gaps, absent, total = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE)
    assert got.splitlines()[0].split("\t") == list(gaps.COPY_COLUMNS) == HEADER
    assert got == text
    assert len(rows) == len((out / "g.gaps.tsv").read_text().splitlines()) - 2  # one line per gap of gaps.tsv
    assert got.splitlines()[-1].endswith(f"absent {absent} of {total} sampled") and 0 <= absent < total
    row = row_of(rows, gap_over(cut_gaps, names[1], B.COPY_TO, B.COPY_TO + B.COPY_BP))
    print("the copy's gap:", row)
    assert row["class"] == "repeat" and row["copies_own_median"] == 2 and row["single_all"] == 0 and row["sampled"] >= 100
    assert row["copies_any_median"] == 2 and row["single_own"] * 2 < row["sampled"]


def test_the_inversion_family_file_equals_a_recomputation_and_the_inversion_is_unique(runs):
    _, families, dirs = runs
    paths, fam = families["inv"]
    names = [os.path.basename(p) for p in paths]
    out = dirs["alone"]
    got = (out / "g.gap_copies.tsv").read_text()
    print(got)
    text, rows, cut_gaps, absent, total = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE)
    assert got == text
    assert got.splitlines()[-1].endswith(f"absent {absent} of {total} sampled") and total > 0
    a = L.INVERT_AT
    inverted = [gap_over(cut_gaps, names[1], a + L.INSERT_BP, a + L.INSERT_BP + L.INVERT_BP),               # (genome 1's coordinates: behind its insertion)
                gap_over(cut_gaps, names[0], a, a + L.INVERT_BP), gap_over(cut_gaps, names[2], a, a + L.INVERT_BP)]
    for gap in inverted:
        row = row_of(rows, gap)
        print("a gap of the inverted segment:", row)
        assert row["class"] == "unique" and row["copies_own_median"] == 1 and row["copies_own_max"] == 1 and row["sampled"] >= 100, row
        assert 2 * row["single_all"] > row["sampled"]
    assert "repeat" not in {r[-1] for r in rows}                                # nothing in this family is held twice


def test_the_tool_reproduces_the_file_alone_and_beside_the_link_options(runs):
    tmp, families, dirs = runs
    paths, _ = families["copy"]
    out = dirs["all"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf")]
    quiet = ["--out", os.devnull, "--summary-out", os.devnull]
    r = L._run(tool + quiet + ["--copies-out", str(tmp / "alone.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.tsv").read_bytes() == (out / "g.gap_copies.tsv").read_bytes()
    r = L._run(tool + ["--out", str(tmp / "again.tsv"), "--summary-out", str(tmp / "again_summary.tsv"), "--links-out", str(tmp / "again_links.tsv"),
                       "--block-links-out", str(tmp / "again_block_links.tsv"), "--copies-out", str(tmp / "again_copies.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    for mine, theirs in (("again_copies.tsv", "g.gap_copies.tsv"), ("again_block_links.tsv", "g.gap_block_links.tsv"), ("again_links.tsv", "g.gap_links.tsv"),
                         ("again.tsv", "g.gaps.tsv"), ("again_summary.tsv", "g.gap_summary.tsv")):
        assert (tmp / mine).read_bytes() == (out / theirs).read_bytes(), mine

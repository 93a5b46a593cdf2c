"""Gap block links end to end: `ntSynt --gap-block-links` and `bin/ntsynt_gaps --block-links-out` on a family in which genome 1 carries a
second copy of 6 kbp of its own chr2 -- sequence that lies inside a block of all three genomes -- between two blocks of chr1.  The file is
compared byte for byte with a recomputation from gaps.cut, the oracle's hashes, the run's own .common.bf and a brute force over
dictionaries of the 2n-list rule, which calls nothing of gaps.block_links.  Every test runs under a time limit of its own."""
import faulthandler
import os
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, gaps, synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
U64_MAX = (1 << 64) - 1
COPY_FROM, COPY_BP, COPY_TO = 100_000, 6_000, 90_000       # genome 1 only: its chr2 [100 000, 106 000) once more, in chr1 at 90 000
RATE, MIN_ANCHORS = 16, 4                                   # the switches' defaults
HEADER = ("genome contig start end left_block right_block target_genome target_contig target_start target_end blocks anchors orientation "
          "from to from_t to_t sampled target_hits placement").split()


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def copy_family(outdir):
    "tests/test_gpu_gap_links.py's family without its two edits; genome 1 gets a copy of a segment of its chr2 inserted into its chr1"
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    c = fam[1][0]
    fam[1][0] = np.concatenate([c[:COPY_TO], fam[1][1][COPY_FROM:COPY_FROM + COPY_BP], c[COPY_TO:]])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def recompute(blocks_tsv, common_bf, fam, names, rate, min_anchors):
    "(text of the file, rows, gaps) from gaps.cut, the oracle's hashes, the filter file and the definitions: no GPU, none of gaps.block_links"
    from ntsynt_amd.pipeline import read_bf
    bits, k = read_bf(common_bf)
    table = assess.read_blocks(blocks_tsv)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, cut_merged = gaps.cut(table, records)
    thresh = np.uint64(U64_MAX // rate)
    order = sorted(names)
    n = len(order)
    low = {}                                                                    # genome -> contig -> (positions, hashes) under the threshold
    for name in order:
        low[name] = {}
        for i, c in enumerate(fam[names.index(name)]):
            pos, h0 = O.hash_all(c.tobytes(), k)
            keep = h0 <= thresh
            low[name][f"chr{i + 1}"] = (pos[keep].astype(np.int64), h0[keep])
    # G: the gaps' sampled k-mers (held by the filter); S: their hashes
    gaps_of, g_lists, sampled = {}, [], []
    for name in order:
        gaps_of[name] = [g for g in cut_gaps if g.genome == name]
        held = {contig: np.array([O.bf_contains(bits, h) for h in h0], dtype=bool) for contig, (_, h0) in low[name].items()}
        lst, cnt = [], []
        for q, g in enumerate(gaps_of[name]):
            pos, h0 = low[name][g.contig]
            inside = (pos >= g.start) & (pos + k <= g.end) & held[g.contig]
            lst += [(int(h), q, int(p) - g.start) for p, h in zip(pos[inside], h0[inside])]
            cnt.append(int(inside.sum()))
        g_lists.append(lst)
        sampled.append(cnt)
    members = {h for lst in g_lists for h, _, _ in lst}
    # B: the k-mers of the merged block intervals whose hash is in S (the filter is not asked)
    merged_of, b_lists, hits = {}, [], []
    for name in order:
        merged_of[name] = [m for m in cut_merged if m.genome == name]
        lst, cnt = [], []
        for q, m in enumerate(merged_of[name]):
            pos, h0 = low[name][m.contig]
            inside = np.flatnonzero((pos >= m.start) & (pos + k <= m.end))
            mine = [(int(h0[i]), q, int(pos[i]) - m.start) for i in inside if int(h0[i]) in members]
            lst += mine
            cnt.append(len(mine))
        b_lists.append(lst)
        hits.append(cnt)
    rows = []
    for la, iva, lb, ivb, anchors, fwd, rev, min_a, max_a, min_b, max_b in L.brute_links(g_lists + b_lists, min_anchors):
        if not la < n <= lb:
            continue                                                            # gap to gap, block to block
        gap, target = gaps_of[order[la]][iva], merged_of[order[lb - n]][ivb]
        from_t, to_t = target.start + min_b, target.start + max_b + k
        ids = []
        for r in table:
            if r.genome == target.genome and r.contig == target.contig and r.start < to_t and r.end > from_t and r.block_id not in ids:
                ids.append(r.block_id)
        if target.genome == gap.genome:
            place = "own"
        else:
            place = "flank" if ({gap.left_block, gap.right_block} - {"."}) & set(ids) else "other"
        rows.append([gap.genome, gap.contig, gap.start, gap.end, gap.left_block, gap.right_block, target.genome, target.contig, target.start, target.end,
                     ",".join(ids), anchors, "+" if fwd > rev else "-" if rev > fwd else ".", gap.start + min_a, gap.start + max_a + k, from_t, to_t,
                     sampled[la][iva], hits[lb - n][ivb], place])
    text = "".join("\t".join(str(v) for v in r) + "\n" for r in [HEADER] + rows)
    return text + f"# k {k}, rate {rate}, min_anchors {min_anchors}, filter {bits.size * 8} bits, set {len(members)} hashes\n", rows, cut_gaps


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family and three runs of it: plain, --gap-links, --gap-block-links --benchmark"
    tmp = tmp_path_factory.mktemp("gap_block_links")
    paths, fam = copy_family(str(tmp))
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("plain", []), ("links", ["--gap-links"]), ("block_links", ["--gap-block-links", "--benchmark"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = L._run(ntsynt + paths + L.PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, paths, fam, dirs


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, _, dirs = runs
    plain, with_links, with_both = dirs["plain"], dirs["links"], dirs["block_links"]
    same = sorted(os.listdir(plain))
    assert "g.synteny_blocks.tsv" in same and "g.common.bf" in same
    for name in same:
        assert (plain / name).read_bytes() == (with_both / name).read_bytes() and (plain / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_links)) - set(same)) == ["g.gap_links.tsv", "g.gap_summary.tsv", "g.gaps.tsv"]
    for name in ("g.gaps.tsv", "g.gap_summary.tsv", "g.gap_links.tsv"):
        assert (with_links / name).read_bytes() == (with_both / name).read_bytes() and (with_links / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_both)) - set(os.listdir(with_links))) == ["g.gap_block_links.tsv", "g.stage_times.tsv"]   # (the latter: --benchmark)
    assert not (with_links / "g.gap_block_links.tsv").exists()
    stages = [ln.split("\t")[0] for ln in (with_both / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_links") < stages.index("gap_block_links")


def test_the_file_equals_a_recomputation(runs):
    _, paths, fam, dirs = runs
    names = [os.path.basename(p) for p in paths]
    out = dirs["block_links"]
    got = (out / "g.gap_block_links.tsv").read_text()
    print(got)
    text, rows, cut_gaps = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, MIN_ANCHORS)
    assert got.splitlines()[0].split("\t") == list(gaps.BLOCK_LINK_COLUMNS) == HEADER
    assert got == text
    # the gap over the inserted copy: one line per target genome, all into the one block that holds the original
    a, b = COPY_TO, COPY_TO + COPY_BP
    best = max((g for g in cut_gaps if g.genome == names[1] and g.contig == "chr1"), key=lambda g: min(g.end, b) - max(g.start, a))
    assert min(best.end, b) - max(best.start, a) >= (b - a) * 0.8, best         # the copy lies in ONE gap, not in a block
    mine = [r for r in rows if (r[0], r[1], r[2], r[3]) == (best.genome, best.contig, best.start, best.end)]
    print(f"lines of the copy's gap {best}:")
    for r in mine:
        print("   ", r)
    assert [r[6] for r in mine] == sorted(names) and len(mine) == 3             # exactly three lines, one per target genome
    for r in mine:
        assert r[7] == "chr2" and r[8] <= COPY_FROM and r[9] >= COPY_FROM + COPY_BP, r      # the interval contains the original
        assert "," not in r[10] and r[10] == mine[0][10] and r[10] != "", r                # one block id, the same in all three
        assert r[12] == "+" and r[11] >= MIN_ANCHORS, r
        assert COPY_FROM <= r[15] and r[16] <= COPY_FROM + COPY_BP, r                       # the anchors lie on the original
        assert r[19] == ("own" if r[6] == names[1] else "other"), r
    print(f"anchors of the copy's gap, by target genome: {[r[11] for r in mine]}")
    links = [ln.split("\t") for ln in (out / "g.gap_links.tsv").read_text().splitlines()[1:] if not ln.startswith("#")]
    at = (best.genome, best.contig, str(best.start))
    assert not [f for f in links if (f[0], f[1], f[2]) == at or (f[6], f[7], f[8]) == at]   # gap_links.tsv has no line for that gap


def test_the_tool_reproduces_the_file_and_is_unchanged_without_the_option(runs):
    tmp, paths, _, dirs = runs
    out = dirs["block_links"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf")]
    quiet = ["--out", os.devnull, "--summary-out", os.devnull]
    r = L._run(tool + ["--out", str(tmp / "again.tsv"), "--summary-out", str(tmp / "again_summary.tsv"), "--links-out", str(tmp / "again_links.tsv"),
                       "--block-links-out", str(tmp / "again_block_links.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "again_block_links.tsv").read_bytes() == (out / "g.gap_block_links.tsv").read_bytes()
    assert (tmp / "again_links.tsv").read_bytes() == (out / "g.gap_links.tsv").read_bytes()
    assert (tmp / "again.tsv").read_bytes() == (out / "g.gaps.tsv").read_bytes()
    assert (tmp / "again_summary.tsv").read_bytes() == (out / "g.gap_summary.tsv").read_bytes()
    r = L._run(tool + quiet + ["--block-links-out", str(tmp / "alone.tsv")], tmp)               # without --links-out
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.tsv").read_bytes() == (out / "g.gap_block_links.tsv").read_bytes()
    before = set(os.listdir(tmp))
    r = L._run(tool, tmp)                                                                       # without the option: what it wrote before
    assert r.returncode == 0 and r.stdout == (out / "g.gaps.tsv").read_text() + (out / "g.gap_summary.tsv").read_text(), r.stderr[-3000:]
    assert set(os.listdir(tmp)) == before
    # other settings through the tool: every held k-mer sampled, a link from one anchor on
    r = L._run(tool + quiet + ["--block-links-out", str(tmp / "dense.tsv"), "--links-rate", "1", "--links-min", "1"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    dense = (tmp / "dense.tsv").read_text().splitlines()
    assert dense[-1].startswith("# k 24, rate 1, min_anchors 1, filter ") and dense[-1].endswith(" hashes")
    assert len(dense) >= len((out / "g.gap_block_links.tsv").read_text().splitlines())

"""`ntSynt --gap-copy-sites` and `bin/ntsynt_gaps --copy-sites-out` end to end (ntsynt_amd/gaps.py copy_sites;
docs/design/04_13_gap_copy_sites.md): on tests/test_gpu_gap_block_links.py's family (a 6 kbp copy of genome 1's chr2 inserted into its
chr1) and tests/test_gpu_gap_links.py's (an inverted segment, a private insertion) the file is recomputed byte for byte on the CPU --
gaps.cut, O.hash_all of every record, the run's filter file, a Counter, tests/sites_brute.py's definitions -- and the copy's gap must
have a `self` line and an `own` line into the block that holds the original, the inversion's gap an `other` line into each other genome
on the other strand; cap 1 takes the copy's lines away; the tool gives the same bytes; a run without the switch is what it was.  Every
test runs under a time limit of its own."""
import faulthandler
import os
import sys
from collections import Counter

import numpy as np
import pytest

from ntsynt_amd import assess, gaps
from oracle import nts_oracle as O
from tests import test_gpu_gap_block_links as B
from tests import test_gpu_gap_links as L
from tests.sites_brute import brute_sites, samples
from tests.test_gpu_gap_copies import gap_over

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
U64_MAX = (1 << 64) - 1
RATE, CAP, STEP, MIN_HITS = 16, 16, 1000, 4                  # the switches' defaults
HEADER = ("genome contig start end left_block right_block class target_genome target_contig from_t to_t blocks hits orientation from to sampled "
          "usable placement").split()


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


_inputs = {}


def inputs(blocks_tsv, common_bf, fam, names, rate):
    "what every cap shares, once per run: the table, the gaps, per genome the k-mers under the threshold, the gaps' sampled records, S and the counts"
    key = (blocks_tsv, rate)
    if key in _inputs:
        return _inputs[key]
    from ntsynt_amd.pipeline import read_bf
    bits, k = read_bf(common_bf)
    table = assess.read_blocks(blocks_tsv)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, _ = gaps.cut(table, records)
    thresh = np.uint64(U64_MAX // rate)
    order = sorted(names)
    low = {}                                                                    # genome -> [(positions, hashes) under the threshold] per record
    for name in order:
        low[name] = []
        for c in fam[names.index(name)]:
            pos, h0 = O.hash_all(c.tobytes(), k)
            keep = h0 <= thresh
            low[name].append((pos[keep].astype(np.int64), h0[keep]))
    gaps_of, lists = {}, []                                                     # G: the gaps' sampled k-mers (held by the filter), per genome [(hash, gap, offset)]
    for name in order:
        gaps_of[name] = [g for g in cut_gaps if g.genome == name]
        held = [np.array([O.bf_contains(bits, h) for h in h0], dtype=bool) for _, h0 in low[name]]
        lst = []
        for q, g in enumerate(gaps_of[name]):
            rec = int(g.contig[3:]) - 1
            pos, h0 = low[name][rec]
            inside = (pos >= g.start) & (pos + k <= g.end) & held[rec]
            lst += [(int(h), q, int(p) - g.start) for p, h in zip(pos[inside], h0[inside])]
        lists.append(lst)
    members = {h for lst in lists for h, _, _ in lst}                           # S
    times = {name: Counter(h for _, h0 in low[name] for h in h0.tolist() if h in members) for name in order}   # c_t(h), genome-wide
    _inputs[key] = (bits, k, table, cut_gaps, order, low, gaps_of, lists, members, times)
    return _inputs[key]


def recompute(blocks_tsv, common_bf, fam, names, rate, cap, step, min_hits):
    "(text of the file, rows as dicts, gaps) from the definitions: no GPU, none of gaps.copy_sites"
    bits, k, table, cut_gaps, order, low, gaps_of, lists, members, times = inputs(blocks_tsv, common_bf, fam, names, rate)
    q_lists = [samples(lst) for lst in lists]
    found, over_cap, total = [], 0, 0
    for ti, t in enumerate(order):
        c = times[t]
        occ = [(h, rec, p) for rec, (pos, h0) in enumerate(low[t]) for p, h in zip(pos.tolist(), h0.tolist()) if h in members and 1 <= c[h] <= cap]     # O_t
        for li, gap, rec, hits, fwd, rev, lo, hi, first, last in brute_sites(q_lists, samples(occ), step, min_hits):
            found.append((li, gap, ti, rec, first, last, hits, fwd, rev, lo, hi))
        over_cap += sum(c[h] > cap for lst in lists for h, _, _ in lst)
        total += sum(len(lst) for lst in lists)
    rows = []
    for li, gap, ti, rec, first, last, hits, fwd, rev, lo, hi in sorted(found):
        g, t, contig = gaps_of[order[li]][gap], order[ti], f"chr{rec + 1}"
        mine = [h for h, q, _ in lists[li] if q == gap]
        own = [times[g.genome][h] for h in mine]
        single_all = sum(all(times[x][h] == 1 for x in order) for h in mine)
        kind = "unique" if 2 * single_all > len(mine) else "repeat" if 2 * (len(mine) - sum(x == 1 for x in own)) > len(mine) else "mixed"
        from_t, to_t = first, last + k
        ids = []
        for r in table:
            if r.genome == t and r.contig == contig and r.start < to_t and r.end > from_t and r.block_id not in ids:
                ids.append(r.block_id)
        if t != g.genome:
            place = "other"
        else:
            place = "self" if contig == g.contig and from_t < g.end and to_t > g.start else "own"
        rows.append([g.genome, g.contig, g.start, g.end, g.left_block, g.right_block, kind, t, contig, from_t, to_t, ",".join(ids) or ".", hits,
                     "+" if fwd > rev else "-" if rev > fwd else ".", g.start + lo, g.start + hi + k, len(mine), sum(1 <= times[t][h] <= cap for h in mine), place])
    text = "".join("\t".join(str(v) for v in r) + "\n" for r in [HEADER] + rows)
    footer = (f"# k {k}, rate {rate}, cap {cap}, step {step}, min_hits {min_hits}, filter {bits.size * 8} bits, set {len(members)} hashes, "
              f"over_cap {over_cap} of {total}\n")
    return text + footer, [dict(zip(HEADER, r)) for r in rows], cut_gaps


def lines_of(rows, gap):
    return [r for r in rows if (r["genome"], r["contig"], r["start"], r["end"]) == (gap.genome, gap.contig, gap.start, gap.end)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the copy family with --gap-block-links --gap-copies and with --gap-copy-sites beside them; the inversion family with --gap-copy-sites alone"
    tmp = tmp_path_factory.mktemp("gap_copy_sites")
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    families, dirs = {}, {}
    for fam_name, build in (("copy", B.copy_family), ("inv", L.gap_family)):
        (tmp / fam_name).mkdir()
        families[fam_name] = build(str(tmp / fam_name))
    for name, fam_name, extra in (("copies", "copy", ["--gap-block-links", "--gap-copies"]),
                                  ("all", "copy", ["--gap-block-links", "--gap-copies", "--gap-copy-sites", "--benchmark"]), ("alone", "inv", ["--gap-copy-sites"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = L._run(ntsynt + families[fam_name][0] + L.PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    return tmp, families, dirs


def test_the_switch_adds_one_file_and_changes_none(runs):
    _, _, dirs = runs
    without, with_all, alone = dirs["copies"], dirs["all"], dirs["alone"]
    same = sorted(os.listdir(without))
    assert "g.synteny_blocks.tsv" in same and "g.gap_copies.tsv" in same and "g.gap_copy_sites.tsv" not in same
    for name in same:                                                           # g.gap_copies.tsv among them
        assert (without / name).read_bytes() == (with_all / name).read_bytes() and (without / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_all)) - set(same)) == ["g.gap_copy_sites.tsv", "g.stage_times.tsv"]   # (the latter: --benchmark)
    stages = [ln.split("\t")[0] for ln in (with_all / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("gaps") < stages.index("gap_block_links") < stages.index("gap_copies") < stages.index("gap_copy_sites")
    listing = set(os.listdir(alone))                                            # the switch alone implies --gap-copies: its file is written, neither link file
    assert {"g.gaps.tsv", "g.gap_summary.tsv", "g.gap_copies.tsv", "g.gap_copy_sites.tsv"} <= listing
    assert not {"g.gap_links.tsv", "g.gap_block_links.tsv", "g.stage_times.tsv"} & listing


def test_the_copy_family_file_equals_a_recomputation_and_the_copy_is_found(runs):
    """the gap over the inserted copy: one `self` line (its own k-mers, where they were taken) and one `own` line into chr2, inside the
    block that holds the original, on the same strand.  The recomputation gives 246 sampled records, a `self` line of 246 hits, an `own`
    line of 246 hits into chr2 100 016 - 105 985 (block 2) and `other` lines of 243 hits (docs/design/04_13_gap_copy_sites.md); the
    figures are printed."""
    _, families, dirs = runs
    paths, fam = families["copy"]
    names = [os.path.basename(p) for p in paths]
    out = dirs["all"]
    got = (out / "g.gap_copy_sites.tsv").read_text()
    print(got)
    text, rows, cut_gaps = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, CAP, STEP, MIN_HITS)
    assert got.splitlines()[0].split("\t") == list(gaps.SITE_COLUMNS) == HEADER
    assert got == text
    gap = gap_over(cut_gaps, names[1], B.COPY_TO, B.COPY_TO + B.COPY_BP)
    mine = lines_of(rows, gap)
    print("the copy's gap:", mine)
    selfs, owns = [r for r in mine if r["placement"] == "self"], [r for r in mine if r["placement"] == "own"]
    assert len(selfs) == 1 and len(owns) == 1 and all(r["class"] == "repeat" for r in mine)
    assert selfs[0]["hits"] >= selfs[0]["sampled"] >= 100 and selfs[0]["orientation"] == "+" and selfs[0]["blocks"] == "."
    own = owns[0]
    original = gaps.blocks_in_span(assess.read_blocks(str(out / "g.synteny_blocks.tsv")), names[1], "chr2", B.COPY_FROM, B.COPY_FROM + B.COPY_BP)
    assert own["target_contig"] == "chr2" and own["orientation"] == "+" and original and set(own["blocks"].split(",")) <= set(original)
    assert B.COPY_FROM <= own["from_t"] < own["to_t"] <= B.COPY_FROM + B.COPY_BP and own["hits"] >= 100
    assert B.COPY_TO <= own["from"] < own["to"] <= B.COPY_TO + B.COPY_BP
    others = [r for r in mine if r["placement"] == "other"]                     # and the original's place in the two other genomes
    assert {r["target_genome"] for r in others} == {names[0], names[2]} and all(r["target_contig"] == "chr2" and r["orientation"] == "+" for r in others)


def test_the_inversion_family_file_equals_a_recomputation_and_the_inversion_is_found_on_the_other_strand(runs):
    _, families, dirs = runs
    paths, fam = families["inv"]
    names = [os.path.basename(p) for p in paths]
    out = dirs["alone"]
    got = (out / "g.gap_copy_sites.tsv").read_text()
    print(got)
    text, rows, cut_gaps = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, CAP, STEP, MIN_HITS)
    assert got == text
    a = L.INVERT_AT
    gap = gap_over(cut_gaps, names[1], a + L.INSERT_BP, a + L.INSERT_BP + L.INVERT_BP)      # (genome 1's coordinates: behind its insertion)
    mine = lines_of(rows, gap)
    print("the inverted segment's gap:", mine)
    for t in (names[0], names[2]):
        into = [r for r in mine if r["target_genome"] == t]
        assert len(into) == 1 and into[0]["placement"] == "other" and into[0]["orientation"] == "-" and into[0]["hits"] >= 100, into
        assert into[0]["target_contig"] == "chr1" and a <= into[0]["from_t"] < into[0]["to_t"] <= a + L.INVERT_BP
    assert [r["placement"] for r in mine if r["target_genome"] == names[1]] == ["self"]
    assert got.splitlines()[-1].endswith(" of " + str(3 * sum(int(r["sampled"]) for r in
                                                             (dict(zip(gaps.COPY_COLUMNS, ln.split("\t"))) for ln in (out / "g.gap_copies.tsv").read_text().splitlines()[1:-1]))))


def test_cap_1_takes_the_copys_lines_away_and_the_tool_reproduces_the_files(runs):
    tmp, families, dirs = runs
    paths, fam = families["copy"]
    names = [os.path.basename(p) for p in paths]
    out = dirs["all"]
    tool = [sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(out / "g.synteny_blocks.tsv"), "--fastas"] + paths + \
           ["--common", str(out / "g.common.bf")]
    quiet = ["--out", os.devnull, "--summary-out", os.devnull]
    # the tool alone, and with cap 1
    r = L._run(tool + quiet + ["--copy-sites-out", str(tmp / "alone.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp / "alone.tsv").read_bytes() == (out / "g.gap_copy_sites.tsv").read_bytes()
    r = L._run(tool + quiet + ["--copy-sites-out", str(tmp / "cap1.tsv"), "--sites-cap", "1"], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    got = (tmp / "cap1.tsv").read_text()
    print(got)
    text, rows, cut_gaps = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, 1, STEP, MIN_HITS)
    assert got == text                                                          # over_cap in the footer included
    _, rows16, _ = recompute(str(out / "g.synteny_blocks.tsv"), str(out / "g.common.bf"), fam, names, RATE, CAP, STEP, MIN_HITS)
    over = [int(t.splitlines()[-1].split("over_cap ")[1].split(" ")[0]) for t in (got, (out / "g.gap_copy_sites.tsv").read_text())]
    gap = gap_over(cut_gaps, names[1], B.COPY_TO, B.COPY_TO + B.COPY_BP)
    mine = lines_of(rows, gap)
    print("the copy's gap at cap 1:", mine, "over_cap at cap 1 and 16:", over)
    assert not [r for r in mine if r["target_genome"] == names[1]]              # its hashes occur twice in its own genome: no `own` line, no `self` line
    assert {r["placement"] for r in lines_of(rows16, gap)} == {"self", "own", "other"}
    assert over[0] > over[1] and over[0] >= 2 * 100
    # beside the other --*-out options: every file is the run's
    r = L._run(tool + ["--out", str(tmp / "again.tsv"), "--summary-out", str(tmp / "again_summary.tsv"), "--links-out", str(tmp / "again_links.tsv"),
                       "--block-links-out", str(tmp / "again_block_links.tsv"), "--copies-out", str(tmp / "again_copies.tsv"),
                       "--copy-sites-out", str(tmp / "again_sites.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    for mine, theirs in (("again_sites.tsv", "g.gap_copy_sites.tsv"), ("again_copies.tsv", "g.gap_copies.tsv"), ("again_block_links.tsv", "g.gap_block_links.tsv"),
                         ("again_links.tsv", "g.gap_links.tsv"), ("again.tsv", "g.gaps.tsv"), ("again_summary.tsv", "g.gap_summary.tsv")):
        assert (tmp / mine).read_bytes() == (out / theirs).read_bytes(), mine


def test_the_switch_is_refused_under_several_ranks_and_without_a_filter(tmp_path):
    "argument parsing: no GPU work"
    paths = []
    for name in ("a.fa", "b.fa"):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w", encoding="utf-8") as fh:
            fh.write(">x\nACGT\n")
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "--gap-copy-sites"]
    r = L._run(ntsynt + ["--no-common"], tmp_path)
    assert r.returncode == 2 and "--gap-copy-sites reads the common Bloom filter: not with --no-common" in r.stderr
    r = L._run(ntsynt, tmp_path, env=dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and "--gap-copy-sites works from the genomes resident on one GPU" in r.stderr and "--copy-sites-out" in r.stderr

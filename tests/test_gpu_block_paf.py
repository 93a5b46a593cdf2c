"""`ntSynt --block-paf` and `bin/ntsynt_block_stats --paf-out` end to end (ntsynt_amd/assess.py block_alignments;
docs/design/04_22_block_alignments.md) on the family of tests/test_gpu_block_end_variants.py -- three genomes of 2 x 60 kbp at 1 %
substitutions, inversions of 8 kbp in genome 1, genome 2's second record reverse-complemented, an unrelated tail, a run of N -- with four
more indels in genome 2's first record, of 40 and 33 bases (beyond the band of 31 diagonals) and of 9 and 6.  The run is --block-paf
--identity-max-edits 1023 --block-ends.  Every record passes tests/cigar_brute.apply_cigar on the target and query substrings its own
coordinates name, read from the FASTA files (the query reverse-complemented for `-`); per pair the NM add up to `edits` of
block_identity.tsv plus left_edits + right_edits of block_ends.tsv, and the first record's tstart and the last one's tend are
ext_start_a and ext_end_a; the file equals a CPU recomputation from the brute modules' segments, distances, extensions and canonical
scripts, encoded by tests/cigar_brute.py; the tool reproduces the file; every other file is byte-equal to that of the same run without
--block-paf.  A second run without --block-ends and with E = 0 shows the chains breaking at the planted indels of 32 bases or more.
Every test runs under a time limit of its own."""
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, synth
from oracle import nts_oracle as O
from oracle import synteny_oracle as SO
from tests import cigar_brute as CB
from tests import extend_brute as X
from tests import identity_brute as B
from tests import variants_brute as V
from tests import wide_brute as W
from tests.test_gpu_block_end_variants import DELETED, INSERTED, N_AT, N_BASES, ORACLE, PARAMS, SPANS, UNRELATED_FROM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 600
K, RATE, BAND, MAX_LEN, MAX_EDITS = 21, 16, 31, 4096, 1023
ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY = 1500, 255, 6
SWITCHES = ["--block-identity", "--identity-max-edits", str(MAX_EDITS), "--block-ends", "--ends-max-len", str(ENDS_MAX_LEN), "--benchmark"]
# genome 2, record 1 (far from the inversion at 24 000 .. 32 000): (position, bases, deleted?) -- from the right
INDELS = ((50_000, 40, True), (45_000, 33, False), (12_000, 9, True), (8_000, 6, False))


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def paf_family(outdir):
    "(paths, genomes): variants_family of tests/test_gpu_block_end_variants.py with INDELS planted in genome 2's first record"
    anc = synth.make_ancestor(120_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    rng = np.random.default_rng(121)
    for rec, lo, hi in SPANS:
        fam[1][rec][lo:hi] = synth.revcomp(fam[1][rec][lo:hi])
    fam[2][1][UNRELATED_FROM:] = synth.random_dna(fam[2][1].size - UNRELATED_FROM, rng)
    fam[0][1][N_AT:N_AT + N_BASES] = ord("N")
    for rec, lo, hi in SPANS:                                 # genome 2: from the right, so that the earlier positions hold
        c = fam[2][rec]
        for at, deleted in ((hi - 350, False), (hi - 800, True), (lo + 800, False), (lo + 350, True)):
            c = np.concatenate([c[:at], c[at + DELETED:]]) if deleted else np.concatenate([c[:at], synth.random_dna(INSERTED, rng), c[at:]])
        fam[2][rec] = c
    c = fam[2][0]
    for at, size, deleted in INDELS:
        c = np.concatenate([c[:at], c[at + size:]]) if deleted else np.concatenate([c[:at], synth.random_dna(size, rng), c[at:]])
    fam[2][0] = c
    fam[2][1] = synth.revcomp(fam[2][1])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def read_fasta(path):
    "{contig: ASCII uint8 array} of a FASTA file"
    out, name = {}, None
    with open(path, "r", encoding="utf-8") as fh:
        for line in fh:
            if line.startswith(">"):
                name = line[1:].split()[0]
                out[name] = []
            else:
                out[name].append(line.strip())
    return {k: np.frombuffer("".join(v).encode(), dtype=np.uint8) for k, v in out.items()}


def recompute(blocks_tsv, fam, names, max_edits, with_ends):
    """the PAF text from the brute forces alone: no GPU, nothing of assess but read_blocks.  A flipped pair is worked in the frame of the
    whole record's reverse complement, where B runs like A, and only the final coordinates are mapped back."""
    genomes = {name: {f"chr{i + 1}": c for i, c in enumerate(contigs)} for name, contigs in zip(names, fam)}
    table = assess.read_blocks(blocks_tsv)
    if max_edits:
        _, facts, _ = W.brute_file_wide(table, genomes, O.hash_all, K, RATE, BAND, MAX_LEN, max_edits)
    else:
        _, facts = B.brute_file(table, genomes, O.hash_all, K, RATE, BAND, MAX_LEN)
    line_of = {(r.block_id, r.genome): r for r in table}
    out, chains_per_pair = [], {}
    for (block, name_a, name_b), (row, results) in facts.items():
        ra, rb = line_of[(block, name_a)], line_of[(block, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        flip = ra.strand != rb.strand
        start_a, len_b = min(max(ra.start, 0), seq_a.size), row["length_b"]
        b_lo = min(max(rb.start, 0), seq_b.size)
        frame_b = X.revcomp(seq_b) if flip else seq_b
        start_b = seq_b.size - b_lo - len_b if flip else b_lo     # the interval's start in B's frame
        groups = []                                           # maximal runs of consecutive aligned segments
        for q, (seg, d) in enumerate(results):
            if d >= B.INVALID:
                continue
            if groups and groups[-1][-1] == q - 1:
                groups[-1].append(q)
            else:
                groups.append([q])
        chains_per_pair[(block, name_a, name_b)] = len(groups)
        pieces, scripts, spans = [], [], []
        for c, members in enumerate(groups):
            first_seg, last_seg = results[members[0]][0], results[members[-1]][0]
            lo_a, lo_b = start_a + first_seg[1], start_b + first_seg[3]
            hi_a, hi_b = start_a + last_seg[1] + last_seg[2], start_b + last_seg[3] + last_seg[4]
            if with_ends and c == 0:                          # backwards from the base in front of the left end point
                n, m = min(ENDS_MAX_LEN, lo_a), min(ENDS_MAX_LEN, lo_b)
                a, b = seq_a[lo_a - n:lo_a][::-1], frame_b[lo_b - m:lo_b][::-1]
                (ext_a, ext_b, edits, _, _), _ = X.extend_brute(a, b, ENDS_PENALTY, ENDS_MAX_EDITS)
                pieces.append((c, ext_a, ext_b, CB.REVERSED))
                scripts.append(V.script(a[:ext_a], b[:ext_b]))
                assert len(scripts[-1]) == edits
                lo_a, lo_b = lo_a - ext_a, lo_b - ext_b
            for q in members:
                seg, d = results[q]
                a, b = seq_a[start_a + seg[1]:start_a + seg[1] + seg[2]], frame_b[start_b + seg[3]:start_b + seg[3] + seg[4]]
                pieces.append((c, seg[2], seg[4], 0))
                scripts.append(V.script(a, b))
                assert len(scripts[-1]) == d
            if with_ends and c == len(groups) - 1:
                n, m = min(ENDS_MAX_LEN, seq_a.size - hi_a), min(ENDS_MAX_LEN, frame_b.size - hi_b)
                a, b = seq_a[hi_a:hi_a + n], frame_b[hi_b:hi_b + m]
                (ext_a, ext_b, edits, _, _), _ = X.extend_brute(a, b, ENDS_PENALTY, ENDS_MAX_EDITS)
                pieces.append((c, ext_a, ext_b, 0))
                scripts.append(V.script(a[:ext_a], b[:ext_b]))
                assert len(scripts[-1]) == edits
                hi_a, hi_b = hi_a + ext_a, hi_b + ext_b
            spans.append((lo_a, hi_a, lo_b, hi_b))
        ops = [(t, p, q, op) for t, s in enumerate(scripts) for op, p, q in s]
        first = np.concatenate([[0], np.cumsum([len(s) for s in scripts])]).astype(np.int64)
        entries, records = CB.brute_cigar(pieces, ops, first, len(groups))
        for c, (rec, (lo_a, hi_a, lo_b, hi_b)) in enumerate(zip(records, spans)):
            q_from, q_to = (seq_b.size - hi_b, seq_b.size - lo_b) if flip else (lo_b, hi_b)
            nm = rec["x"] + rec["ins"] + rec["del"]
            out.append("\t".join(str(v) for v in (rb.contig, seq_b.size, q_from, q_to, "-" if flip else "+", ra.contig, seq_a.size, lo_a, hi_a, rec["eq"],
                                                  rec["eq"] + nm, 255, f"NM:i:{nm}", f"bi:i:{block}", f"tg:Z:{name_a}", f"qg:Z:{name_b}", f"ch:i:{c}",
                                                  "cg:Z:" + CB.cigar_string(entries[rec["first"]:rec["first"] + rec["n_cig"]]))))
    return "".join(line + "\n" for line in out), chains_per_pair


def _run(cmd, cwd, **env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT, **env))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    "the family, the oracle's table, the recomputations; three runs: without --block-paf, with it, and --block-paf alone (E = 0, no ends)"
    tmp = tmp_path_factory.mktemp("paf_runs")
    paths, fam = paf_family(str(tmp))
    (tmp / "oracle").mkdir()
    cwd = os.getcwd()
    try:
        os.chdir(tmp / "oracle")
        table = SO.run_pipeline(paths, **ORACLE).outputs["g.synteny_blocks.tsv"]
    finally:
        os.chdir(cwd)
    (tmp / "oracle" / "table.tsv").write_text(table)
    names = [os.path.basename(p) for p in paths]
    want = {"full": recompute(str(tmp / "oracle" / "table.tsv"), fam, names, MAX_EDITS, True),
            "narrow": recompute(str(tmp / "oracle" / "table.tsv"), fam, names, 0, False)}
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    dirs = {}
    for name, extra in (("without", SWITCHES), ("full", SWITCHES + ["--block-paf"]), ("narrow", ["--block-paf"])):
        dirs[name] = tmp / name
        dirs[name].mkdir()
        r = _run(ntsynt + paths + PARAMS + extra, dirs[name])
        assert r.returncode == 0, r.stderr[-3000:]
    assert (dirs["full"] / "g.synteny_blocks.tsv").read_text() == table
    return tmp, paths, dirs, want


def records_of(text):
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        assert len(f) == 18 and [t[:5] for t in f[12:]] == list(assess.PAF_TAGS), line[:200]
        out.append(dict(q=f[0], q_len=int(f[1]), q_from=int(f[2]), q_to=int(f[3]), sign=f[4], t=f[5], t_len=int(f[6]), t_from=int(f[7]), t_to=int(f[8]),
                        matches=int(f[9]), columns=int(f[10]), nm=int(f[12][5:]), block=f[13][5:], tg=f[14][5:], qg=f[15][5:], ch=int(f[16][5:]), cg=f[17][5:]))
    return out


def tsv_rows(text):
    lines = text.splitlines()
    columns = lines[0].split("\t")
    return [dict(zip(columns, ln.split("\t"))) for ln in lines[1:] if not ln.startswith("#")]


def test_every_record_passes_apply_cigar_on_the_fasta_files(runs):
    _, paths, dirs, _ = runs
    genomes = {os.path.basename(p): read_fasta(p) for p in paths}
    records = records_of((dirs["full"] / "g.block_alignments.paf").read_text())
    assert len(records) >= 6 and {r["sign"] for r in records} == {"+", "-"}
    seen, most = set(), {"I": 0, "D": 0}
    for r in records:
        target, query = genomes[r["tg"]][r["t"]], genomes[r["qg"]][r["q"]]
        assert (r["t_len"], r["q_len"]) == (target.size, query.size)
        query = query[r["q_from"]:r["q_to"]]
        eq, x, ins, dele = CB.apply_cigar(target[r["t_from"]:r["t_to"]], X.revcomp(query) if r["sign"] == "-" else query, r["cg"])
        assert (r["matches"], r["columns"], r["nm"]) == (eq, eq + x + ins + dele, x + ins + dele), r
        seen |= {letter for _, letter in CB.parse_cigar(r["cg"])}
        most = {"I": max(most["I"], ins), "D": max(most["D"], dele)}
    # the planted indels of 40 and 33 bases lie inside chains (chance matches may split an indel of random bases into several runs)
    assert seen == set("=XID") and most["I"] >= 33 and most["D"] >= 33, (seen, most)


def test_per_pair_sums_and_breakpoints(runs):
    _, _, dirs, _ = runs
    records = records_of((dirs["full"] / "g.block_alignments.paf").read_text())
    identity = {(r["block_id"], r["genome_a"], r["genome_b"]): r for r in tsv_rows((dirs["full"] / "g.block_identity.tsv").read_text())}
    ends = {(r["block_id"], r["genome_a"], r["genome_b"]): r for r in tsv_rows((dirs["full"] / "g.block_ends.tsv").read_text())}
    by_pair = {}
    for r in records:
        by_pair.setdefault((r["block"], r["tg"], r["qg"]), []).append(r)
    assert list(by_pair) == [key for key in identity if int(identity[key]["aligned"]) > 0]            # block_identity.tsv's order
    for key, mine in by_pair.items():
        assert [r["ch"] for r in mine] == list(range(len(mine))) and [r["t_from"] for r in mine] == sorted(r["t_from"] for r in mine)
        assert sum(r["nm"] for r in mine) == int(identity[key]["edits"]) + int(ends[key]["left_edits"]) + int(ends[key]["right_edits"]), key
        assert (mine[0]["t_from"], mine[-1]["t_to"]) == (int(ends[key]["ext_start_a"]), int(ends[key]["ext_end_a"])), key
        q_lo, q_hi = min(r["q_from"] for r in mine), max(r["q_to"] for r in mine)
        assert (q_lo, q_hi) == (int(ends[key]["ext_start_b"]), int(ends[key]["ext_end_b"])), key


def test_the_file_equals_the_recomputation(runs):
    _, _, dirs, want = runs
    got = (dirs["full"] / "g.block_alignments.paf").read_text()
    text, _ = want["full"]
    assert got.count("\n") == text.count("\n")
    assert got == text, [(g[:150], w[:150]) for g, w in zip(got.splitlines(), text.splitlines()) if g != w][:2]


def test_the_tool_reproduces_the_file(runs):
    tmp, paths, dirs, want = runs
    out, ends_out = tmp / "tool.block_alignments.paf", tmp / "tool.block_ends.tsv"
    fais = [str(dirs["full"] / (os.path.basename(p) + ".fai")) for p in paths]
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(dirs["full"] / "g.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--paf-out", str(out), "--identity-max-edits", str(MAX_EDITS), "--ends-out", str(ends_out), "--ends-max-len",
                                     str(ENDS_MAX_LEN), "--divergence-out", str(tmp / "tool.div.tsv")], tmp)
    assert r.returncode == 0, r.stderr[-3000:]
    assert out.read_bytes() == (dirs["full"] / "g.block_alignments.paf").read_bytes()
    assert ends_out.read_bytes() == (dirs["full"] / "g.block_ends.tsv").read_bytes()


def test_every_other_file_is_that_of_the_run_without_the_switch(runs):
    _, _, dirs, _ = runs
    same = sorted(os.listdir(dirs["without"]))
    assert "g.block_ends.tsv" in same and "g.block_identity.tsv" in same and not [n for n in same if n.endswith(".paf")]
    for name in same:
        if name != "g.stage_times.tsv":
            assert (dirs["without"] / name).read_bytes() == (dirs["full"] / name).read_bytes(), name
    assert sorted(set(os.listdir(dirs["full"])) - set(same)) == ["g.block_alignments.paf"]
    stages = {name: [ln.split("\t")[0] for ln in (dirs[name] / "g.stage_times.tsv").read_text().splitlines()] for name in ("without", "full")}
    assert "block_paf" in stages["full"] and "block_paf:cigar_atoms" in stages["full"] and "block_paf:cigar_merge" in stages["full"]
    assert [s for s in stages["full"] if not s.startswith("block_paf")] == stages["without"]


def test_without_ends_and_wide_pass_the_chains_break_at_the_large_indels(runs):
    _, _, dirs, want = runs
    text, chains_narrow = want["narrow"]
    _, chains_full = want["full"]
    got = (dirs["narrow"] / "g.block_alignments.paf").read_text()
    assert got == text, [(g[:150], w[:150]) for g, w in zip(got.splitlines(), text.splitlines()) if g != w][:2]
    assert not [n for n in os.listdir(dirs["narrow"]) if "block_identity" in n or "block_ends" in n]        # (the switch works alone)
    broken = [key for key in chains_full if chains_narrow[key] > chains_full[key]]
    assert broken and all("fam2.fa" in key[1:] for key in broken), (chains_narrow, chains_full)
    for r in records_of(got):
        assert all(length < 32 for length, letter in CB.parse_cigar(r["cg"]) if letter in "ID"), r["cg"][:200]

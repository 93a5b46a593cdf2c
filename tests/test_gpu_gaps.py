"""Gap content on the GPU: nts_bf_count_intervals (csrc/nts_bf_iv.inc) against the oracle -- O.hash_all of the record, a position
filter per interval, O.bf_contains per k-mer -- bit for bit; the launch cut forced on the experiments build; `ntSynt --gaps` and
bin/ntsynt_gaps end to end against an independent recomputation from gaps.cut, the oracle and the run's own .common.bf.  Every test
runs under a time limit of its own (a hung call ends the process, with a traceback).

_oracle_inputs() and the `0 < hits < kmers` condition need no GPU: tests/test_gaps_oracle_inputs.py checks them on the CPU."""
import faulthandler
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, gaps, synth
from oracle import nts_oracle as O
from tests.helpers import END_CASE_KMERS, genome_end_case, oracle_counts, random_records, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
FILTER_BYTES = 1 << 19            # 4.2 M bits for 0.3 M k-mers: occupancy about 7 %
SUBSTITUTIONS = 0.02              # synth.derive_genome's pairwise figure: 1 % of the bases of the copy differ (0.99^150 = 22 % of the 150-mers survive)


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def oracle_inputs():
    "(names, records, the mutated copy's records): N runs, lower case, records shorter than any k and shorter than most"
    rng = np.random.default_rng(49)
    seqs = random_records(rng, [150_000, 40_000, 70_000, 9, 100, 20_000], n_frac=0.02, lower_frac=0.1)
    seqs.insert(3, b"N" * 3000)
    copy = synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=77, structural=False)
    return [f"r{i}" for i in range(len(seqs))], seqs, [c.tobytes() for c in copy]


def intervals_for(k, seqs):
    iv = [(0, a, a + 10_000) for a in range(0, 150_000, 10_000)]             # tile record 0
    iv += [(1, 0, 40_000),                                                     # a whole record
           (2, 50_000, 10**12),                                                # ends beyond the record
           (2, 0, 30_000), (2, 20_000, 60_000), (0, 5_000, 95_000),            # overlapping, not in order
           (0, 100, 100 + k - 1), (1, 700, 700 + k), (1, 900, 900),            # fewer than k bases; one k-mer; empty
           (1, 500, 400),                                                      # end before start
           (3, 0, 3000), (3, 10, 500),                                         # only N
           (4, 0, 9), (5, 0, 100), (5, 200, 300),                              # short records; starts beyond the record
           (6, 0, 20_000), (6, 19_990, 20_000)]
    n_at = [i for i, c in enumerate(seqs[0]) if c == ord("N")]
    assert n_at
    iv.append((0, max(n_at[len(n_at) // 2] - 300, 0), n_at[len(n_at) // 2] + 300))      # crosses an N run
    return iv


def _filter_of(ctx, names, seqs, k, nbytes=FILTER_BYTES):
    from ntsynt_amd.device import BloomFilter
    g = to_device(ctx, names, seqs)
    bf = BloomFilter(ctx, nbytes, k)
    try:
        bf.insert(g)
    finally:
        g.free()
    return bf


@pytest.mark.parametrize("k", KS)
def test_interval_counts_equal_the_oracle(ctx, k):
    names, seqs, copy = oracle_inputs()
    bf = _filter_of(ctx, names, copy, k)
    g = to_device(ctx, names, seqs)
    try:
        bits = bf.to_numpy()
        iv = intervals_for(k, seqs)
        kmers, hits = g.bf_count_intervals(bf, iv, k)
        assert kmers.dtype == np.uint64 and hits.dtype == np.uint64 and kmers.shape == hits.shape == (len(iv),)
        ref = oracle_counts(seqs, k, bits, iv)
        for i, row in enumerate(iv):
            print(f"k {k} {row}: kmers {int(kmers[i])} hits {int(hits[i])} oracle {ref[i]}")
        for i, row in enumerate(iv):
            assert (int(kmers[i]), int(hits[i])) == ref[i], (k, row, int(kmers[i]), int(hits[i]), ref[i])
        total_k, total_h = sum(r[0] for r in ref), sum(r[1] for r in ref)
        assert 0 < total_h < total_k, (k, total_h, total_k)                       # never a vacuous match
        by = dict(zip(iv, ref))
        assert by[(0, 100, 100 + k - 1)] == (0, 0) and by[(1, 900, 900)] == (0, 0) and by[(3, 0, 3000)] == (0, 0) and by[(4, 0, 9)] == (0, 0)
        assert by[(1, 700, 700 + k)][0] <= 1 and by[(5, 200, 300)] == (0, 0) and by[(1, 500, 400)] == (0, 0)
        # whole records: every valid k-mer of the genome once
        whole = [(r, 0, len(s)) for r, s in enumerate(seqs)]
        kmers, hits = g.bf_count_intervals(bf, whole, k)
        assert int(kmers.sum()) == g.valid_kmers(k)
        assert [(int(a), int(b)) for a, b in zip(kmers, hits)] == oracle_counts(seqs, k, bits, whole)
        empty = g.bf_count_intervals(bf, np.zeros((0, 3), np.uint64), k)
        assert empty[0].size == 0 and empty[1].size == 0
        # N bases from the valid stretches
        valid = g.valid_bases(iv)
        for (rec, start, end), v in zip(iv, valid):
            seg = seqs[rec][min(start, len(seqs[rec])):max(min(end, len(seqs[rec])), min(start, len(seqs[rec])))]
            assert int(v) == sum(seg.upper().count(b) for b in (b"A", b"C", b"G", b"T")), (rec, start, end)
    finally:
        g.free()
        bf.free()


@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=79, structural=False)]
    bf = _filter_of(ctx, names, copy, k, nbytes=1 << 16)
    g = to_device(ctx, names, seqs)
    try:
        kmers, hits = g.bf_count_intervals(bf, iv, k)
        ref = oracle_counts(seqs, k, bf.to_numpy(), iv)
        for i, row in enumerate(iv):
            print(f"k {k} {row}: kmers {int(kmers[i])} hits {int(hits[i])} oracle {ref[i]}")
        assert [r[0] for r in ref[:12]] == list(END_CASE_KMERS) * 2 and ref[12][0] == 500 - k + 1 + 460 - k + 1, ref
        assert [(int(a), int(b)) for a, b in zip(kmers, hits)] == ref
        assert 0 < sum(r[1] for r in ref) < sum(r[0] for r in ref)               # never a vacuous match
    finally:
        g.free()
        bf.free()


def test_full_and_empty_filters_and_a_bad_record_index(ctx):
    from ntsynt_amd.device import BloomFilter, NtsError
    names, seqs, _ = oracle_inputs()
    g = to_device(ctx, names, seqs)
    ones = BloomFilter(ctx, FILTER_BYTES, 24, ones=True)
    zero = BloomFilter(ctx, FILTER_BYTES, 24)
    try:
        for k in KS:
            iv = intervals_for(k, seqs)
            kmers, hits = g.bf_count_intervals(ones, iv, k)
            assert kmers.sum() > 0 and np.array_equal(kmers, hits), k
            kmers0, hits0 = g.bf_count_intervals(zero, iv, k)
            assert np.array_equal(kmers0, kmers) and not hits0.any(), k
        with pytest.raises(NtsError, match="record index out of range"):
            g.bf_count_intervals(ones, [(0, 0, 10), (len(seqs), 0, 10)], 24)
    finally:
        g.free()
        ones.free()
        zero.free()


def test_more_tiles_than_one_launch_takes_give_the_same_counts(ctx_x, monkeypatch):
    names, seqs, copy = oracle_inputs()
    k = 24
    bf = _filter_of(ctx_x, names, copy, k)
    g = to_device(ctx_x, names, seqs)
    try:
        iv = intervals_for(k, seqs) + [(0, a, a + 700) for a in range(0, 140_000, 500)]       # many short intervals as well
        ctx_x.profile(2)
        try:
            before = ctx_x.timing("bf_count_iv")[1]
            plain = g.bf_count_intervals(bf, iv, k)
            one = ctx_x.timing("bf_count_iv")[1] - before
            monkeypatch.setenv("NTS_BF_IV_SLICE", "7")
            cut = g.bf_count_intervals(bf, iv, k)
            many = ctx_x.timing("bf_count_iv")[1] - before - one
        finally:
            ctx_x.profile(False)
        print(f"launches: {one} uncut, {many} with 7 tiles per launch")
        assert one == 1 and many > 40
        assert np.array_equal(plain[0], cut[0]) and np.array_equal(plain[1], cut[1])
        ref = oracle_counts(seqs, k, bf.to_numpy(), iv)
        assert [(int(a), int(b)) for a, b in zip(*cut)] == ref
    finally:
        g.free()
        bf.free()


def test_the_launch_knob_is_not_in_the_product_build(ctx, monkeypatch):
    names, seqs, copy = oracle_inputs()
    bf = _filter_of(ctx, names, copy, 24)
    g = to_device(ctx, names, seqs)
    try:
        monkeypatch.setenv("NTS_BF_IV_SLICE", "7")
        ctx.profile(2)
        try:
            before = ctx.timing("bf_count_iv")[1]
            g.bf_count_intervals(bf, intervals_for(24, seqs), 24)
            assert ctx.timing("bf_count_iv")[1] - before == 1
        finally:
            ctx.profile(False)
    finally:
        g.free()
        bf.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
INSERT_AT, INSERT_BP = 90_000, 6_000           # genome 1 only, contig 1: sequence no other genome has
INVERT_AT, INVERT_BP = 200_000, 6_000          # genome 1 only, contig 1 (coordinates before the insertion): shared, but on the other strand
PARAMS = ["-d", "1", "-k", "24", "-w", "300", "--w_rounds", "100", "10", "--indel", "500", "--merge", "1000", "-b", "8000", "-p", "g"]


def gap_family(outdir):
    """three genomes of 2 x 300 kbp at 1 %, no rearrangements but two in genome 1: an insertion of random sequence and an inverted
    segment, both shorter than the shortest block reported (-b 8000), so that neither can be a block of its own"""
    anc = synth.make_ancestor(600_000, 2, seed=21)
    fam = [synth.derive_genome(anc, 0.01, j, seed=21, structural=False) for j in range(3)]
    c = fam[1][0]
    c[INVERT_AT:INVERT_AT + INVERT_BP] = synth.revcomp(c[INVERT_AT:INVERT_AT + INVERT_BP])
    private = synth.random_dna(INSERT_BP, np.random.default_rng(5))
    fam[1][0] = np.concatenate([c[:INSERT_AT], private, c[INSERT_AT:]])
    paths = []
    for j, contigs in enumerate(fam):
        paths.append(os.path.join(outdir, f"fam{j}.fa"))
        synth.write_fasta(paths[-1], contigs)
    return paths, fam


def _run(cmd, cwd, env=None, timeout=900):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env or dict(os.environ, PYTHONPATH=ROOT))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def recompute(blocks_tsv, common_bf, fam, names):
    "both files' texts from gaps.cut, the oracle's hashes and the filter file: no GPU, none of gaps.report"
    from ntsynt_amd.pipeline import read_bf
    bits, k = read_bf(common_bf)
    occ = float(np.unpackbits(bits).sum()) / (bits.size * 8)
    blocks = assess.read_blocks(blocks_tsv)
    records = {name: [(f"chr{i + 1}", int(c.size)) for i, c in enumerate(contigs)] for name, contigs in zip(names, fam)}
    cut_gaps, cut_merged = gaps.cut(blocks, records)
    held = {}
    for name, contigs in zip(names, fam):
        for i, c in enumerate(contigs):
            pos, h0 = O.hash_all(c.tobytes(), k)
            held[(name, f"chr{i + 1}")] = (pos.astype(np.int64), np.array([O.bf_contains(bits, h) for h in h0], dtype=bool), c)

    def rows_of(items):
        out = []
        for r in items:
            pos, hit, c = held[(r.genome, r.contig)]
            inside = (pos >= r.start) & (pos + k <= r.end)
            out.append(dict(r._asdict(), n_bases=int((~np.isin(c[r.start:r.end], np.frombuffer(b"ACGTacgt", dtype=np.uint8))).sum()),
                            kmers=int(inside.sum()), shared_kmers=int(hit[inside].sum())))
        return out
    gap_rows, block_rows = rows_of(cut_gaps), rows_of(cut_merged)
    return (gaps.table(gap_rows, k, bits.size * 8, occ), gaps.summary(gap_rows, block_rows, k, bits.size * 8, occ, genomes=names), gap_rows, k)


def test_ntsynt_gaps_end_to_end(tmp_path):
    paths, fam = gap_family(str(tmp_path))
    names = [os.path.basename(p) for p in paths]
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    plain, with_ = tmp_path / "plain", tmp_path / "gaps"
    plain.mkdir()
    with_.mkdir()
    r = _run(ntsynt + paths + PARAMS, plain)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(ntsynt + paths + PARAMS + ["--gaps", "--benchmark"], with_)
    assert r.returncode == 0, r.stderr[-3000:]
    # without the switch: the same outputs, byte for byte, and no gap files
    expected_same = sorted(n for n in os.listdir(plain))
    assert "g.synteny_blocks.tsv" in expected_same and "g.common.bf" in expected_same
    for name in expected_same:
        assert (plain / name).read_bytes() == (with_ / name).read_bytes() and (plain / name).stat().st_size > 0, name
    assert sorted(set(os.listdir(with_)) - set(expected_same)) == ["g.gap_summary.tsv", "g.gaps.tsv", "g.stage_times.tsv"]
    assert "gaps\t" in (with_ / "g.stage_times.tsv").read_text()
    # every figure of both files, recomputed
    table, summary, gap_rows, k = recompute(str(with_ / "g.synteny_blocks.tsv"), str(with_ / "g.common.bf"), fam, names)
    assert k == 24
    got_table, got_summary = (with_ / "g.gaps.tsv").read_text(), (with_ / "g.gap_summary.tsv").read_text()
    print(got_table)
    print(got_summary)
    assert got_table.splitlines()[0].split("\t") == list(gaps.GAP_COLUMNS) and got_summary.splitlines()[0].split("\t") == list(gaps.SUMMARY_COLUMNS)
    assert got_table == table
    assert got_summary == summary
    assert len(got_summary.splitlines()) == 2 + 2 * 3 and sum(r["kmers"] for r in gap_rows) > 0
    # the private insertion is the genome's own, the inverted segment is shared sequence the chaining dropped
    occ = float(got_table.splitlines()[-1].rsplit(" ", 1)[1])

    def gap_over(a, b):
        best = max((r for r in gap_rows if r["genome"] == names[1] and r["contig"] == "chr1"), key=lambda r: min(r["end"], b) - max(r["start"], a))
        assert min(best["end"], b) - max(best["start"], a) >= (b - a) * 0.8, (a, b, best)      # the segment lies in ONE gap, not in a block
        return best
    ins = gap_over(INSERT_AT, INSERT_AT + INSERT_BP)
    inv = gap_over(INVERT_AT + INSERT_BP, INVERT_AT + INSERT_BP + INVERT_BP)
    e_ins, e_inv = (gaps.excess(r["shared_kmers"], r["kmers"], occ) for r in (ins, inv))
    print(f"insertion gap {ins} excess {e_ins}\ninversion gap {inv} excess {e_inv}\noccupancy {occ}")
    assert ins is not inv and e_ins < e_inv
    # the tool on the finished run reproduces both files byte for byte
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(with_ / "g.synteny_blocks.tsv"), "--fastas"] + paths +
             ["--common", str(with_ / "g.common.bf"), "--out", str(tmp_path / "again.tsv"), "--summary-out", str(tmp_path / "again_summary.tsv")], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "again.tsv").read_bytes() == (with_ / "g.gaps.tsv").read_bytes()
    assert (tmp_path / "again_summary.tsv").read_bytes() == (with_ / "g.gap_summary.tsv").read_bytes()
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_gaps"), "--tsv", str(with_ / "g.synteny_blocks.tsv"), "--fastas"] + paths +
             ["--common", str(with_ / "g.common.bf")], tmp_path)
    assert r.returncode == 0 and r.stdout == got_table + got_summary, r.stderr[-3000:]
    # the stage is listed by --dry-run
    r = _run(ntsynt + paths + PARAMS + ["--gaps", "--assess", "-n"], tmp_path)
    assert r.returncode == 0 and r.stdout.strip().endswith("ntsynt_synteny -> assess -> gaps"), r.stdout[-500:]


def test_gaps_and_assess_together(tmp_path):
    paths, _ = gap_family(str(tmp_path))
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    only, both = tmp_path / "assess", tmp_path / "both"
    only.mkdir()
    both.mkdir()
    r = _run(ntsynt + paths + PARAMS + ["--assess"], only)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(ntsynt + paths + PARAMS + ["--assess", "--gaps", "--benchmark"], both)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("g.block_stats.tsv", "g.block_divergence.tsv", "g.synteny_blocks.tsv"):
        assert (only / name).read_bytes() == (both / name).read_bytes() and (only / name).stat().st_size > 0, name
    for name in ("g.gaps.tsv", "g.gap_summary.tsv"):
        assert (both / name).stat().st_size > 0 and not (only / name).exists(), name
    stages = [ln.split("\t")[0] for ln in (both / "g.stage_times.tsv").read_text().splitlines()]
    assert stages.index("assess") < stages.index("gaps")


def test_gaps_is_refused_under_two_ranks_and_without_a_filter(tmp_path):
    paths = synth.make_family(str(tmp_path), 2, 200_000, 1, 0.01, seed=14)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT, NTS_RCCL_LIB=STANDIN, MASTER_ADDR="127.0.0.1", NTS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "-p", "p", "--gaps"]
    r = _run(cmd, out, env=env, timeout=300)
    assert r.returncode != 0
    assert "--gaps works from the genomes resident on one GPU" in r.stderr
    assert os.listdir(out) == []
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "-p", "p", "--gaps", "--no-common"], out)
    assert r.returncode != 0 and "--gaps reads the common Bloom filter" in r.stderr and os.listdir(out) == []

"""Assessment of synteny blocks on the GPU: nts_minhash_intervals (csrc/nts_minhash_iv.inc) against np.unique over the oracle's hashes
per interval, both retry directions and the chunking forced on the experiments build, nts_minhash_pairs against
divergence.distance's two integers, the per-interval estimate against the substitution rate of the generator, and `ntSynt --assess`
/ bin/ntsynt_block_stats end to end.  Every test runs under a time limit of its own (a hung call ends the process, with a traceback)."""
import faulthandler
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import assess, divergence, synth
from oracle import nts_oracle as O
from tests.divergence_ref import SENTINEL
from tests.helpers import END_CASE_KMERS, genome_end_case, random_records, to_device
from tests.helpers import oracle_sketches as _oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")
STEP_SECONDS = 600


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


@pytest.fixture(scope="module")
def records():
    rng = np.random.default_rng(48)
    r0, r1, r5 = random_records(rng, [120_000, 30_000, 60_000], n_frac=0.02, lower_frac=0.1)
    unit = random_records(rng, [171], n_frac=0, lower_frac=0)[0]
    satellite = unit * 600                                         # 102600 bases, at most 171 distinct k-mers per strand pair
    seqs = [r0, r1, satellite, b"N" * 5000, b"ACGTTGCATGCCAGT", r5]
    return [f"r{i}" for i in range(len(seqs))], seqs


def _intervals(k, s):
    four_s = 4 * s + k - 1
    return [(0, 100, 100 + k - 1),                 # shorter than k
            (1, 500, 500 + k),                     # exactly one k-mer
            (1, 1000, 1000 + four_s),              # 4 s k-mers (where no N falls)
            (1, 2000, 2000 + four_s + 1),          # one more: the threshold applies
            (0, 30000, 30000 + four_s + 500),
            (1, 0, 30_000),                        # a whole record
            (0, 0, 120_000),
            (5, 50_000, 10**12),                   # ends past the record
            (0, 50_000, 90_000), (0, 20_000, 70_000), (5, 100, 40_000), (0, 100, 20_000),     # overlapping, not in order
            (3, 0, 5000), (3, 100, 200),           # only N
            (2, 0, 102_600), (2, 1000, 50_000),    # satellite array: many k-mers, few distinct
            (4, 100, 200), (4, 0, 15),             # starts past the record; a record shorter than most k
            (5, 0, 60_000)]


def _check(g, seqs, k, s, intervals, note=""):
    out, counts, n_kmers = g.minhash_intervals(intervals, k, s)
    ref, ref_nk = _oracle(seqs, k, s, intervals)
    assert out.shape == (len(intervals), s) and counts.dtype == np.uint32 and n_kmers.dtype == np.uint64
    for i, iv in enumerate(intervals):
        assert int(n_kmers[i]) == ref_nk[i], (note, k, s, iv, int(n_kmers[i]), ref_nk[i])
        assert int(counts[i]) == ref[i].size, (note, k, s, iv, int(counts[i]), ref[i].size)
        assert np.array_equal(out[i, :counts[i]], ref[i]), (note, k, s, iv)
    return ref, ref_nk


@pytest.mark.parametrize("k", [21, 24, 64, 150])
def test_interval_sketches_equal_the_oracle(ctx, records, k):
    names, seqs = records
    g = to_device(ctx, names, seqs)
    try:
        for s in (1, 1000, 10_000):
            iv = _intervals(k, s)
            ref, ref_nk = _check(g, seqs, k, s, iv)
            by = dict(zip(iv, zip(ref, ref_nk)))
            assert by[iv[0]][1] == 0 and by[iv[1]][1] <= 1 and by[(3, 0, 5000)][1] == 0 and by[(4, 100, 200)][1] == 0
            if k < 171:
                sat, sat_nk = by[(2, 0, 102_600)]
                assert sat_nk == 102_600 - k + 1 and 0 < sat.size <= 171 and (s < 171 or sat.size < s)
            print(f"k {k} s {s}: passes/chunks/sweeps {ctx.minhash_intervals_stats()}")
        out, counts, n_kmers = g.minhash_intervals(np.zeros((0, 3), np.uint64), k, 100)
        assert out.shape == (0, 100) and counts.size == 0
    finally:
        g.free()


@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    names, seqs, iv = genome_end_case(k)
    g = to_device(ctx, names, seqs)
    try:
        for s in (100, 10_000):                                  # a threshold for the long intervals; every hash of every interval
            ref, ref_nk = _check(g, seqs, k, s, iv, note="genome end")
            assert ref_nk[:12] == list(END_CASE_KMERS) * 2, ref_nk
            assert all(r.size == min(s, n) for r, n in zip(ref[:12], ref_nk[:12])), [r.size for r in ref]      # random sequence: no repeated k-mer
    finally:
        g.free()


def test_bad_record_index_is_refused(ctx, records):
    from ntsynt_amd.device import NtsError
    names, seqs = records
    g = to_device(ctx, names, seqs)
    try:
        with pytest.raises(NtsError, match="record index out of range"):
            g.minhash_intervals([(len(seqs), 0, 10)], 21, 10)
    finally:
        g.free()


def test_whole_record_interval_equals_the_genome_sketch(ctx):
    seq = random_records(np.random.default_rng(5), [400_000], n_frac=0.02, lower_frac=0.1)[0]
    g = to_device(ctx, ["one"], [seq])
    try:
        for k, s in ((21, 1000), (24, 10_000), (150, 1)):
            out, counts, n_kmers = g.minhash_intervals([(0, 0, len(seq))], k, s)
            assert np.array_equal(out[0, :counts[0]], g.minhash(k, s)) and int(n_kmers[0]) == g.valid_kmers(k)
    finally:
        g.free()


def test_both_retry_directions_and_chunks_stay_exact(ctx_x, records, monkeypatch):
    names, seqs = records
    g = to_device(ctx_x, names, seqs)
    try:
        for k, s in ((21, 1000), (64, 100)):
            iv = _intervals(k, s)
            _check(g, seqs, k, s, iv, "plain")
            p0, c0, _ = ctx_x.minhash_intervals_stats()
            assert c0 == 1 and p0 <= 2                          # (thresholds aim at 4 s survivors: one sweep, seldom a second)
            for env, retried, chunked in (({"NTS_MINHASH_TAU0": "1"}, True, False),                                    # far too low: raised
                                          ({"NTS_MINHASH_TAU0": str(2**64 - 1), "NTS_MINHASH_CAP": "16"}, True, False),  # overflows: lowered
                                          ({"NTS_MINHASH_TAU0": str(2**40), "NTS_MINHASH_CAP": "64"}, True, False),
                                          ({"NTS_MINHASH_IV_BUDGET": str(40 * s * 8)}, False, True)):
                for key, val in env.items():
                    monkeypatch.setenv(key, val)
                ctx_x.profile(2)
                before = ctx_x.timing("minhash_iv")[1]
                try:
                    _check(g, seqs, k, s, iv, str(env))
                    launches = ctx_x.timing("minhash_iv")[1] - before
                finally:
                    ctx_x.profile(False)
                    for key in env:
                        monkeypatch.delenv(key)
                passes, chunks, sweeps = ctx_x.minhash_intervals_stats()
                print(f"k {k} s {s} {env}: passes {passes}, chunks {chunks}, sweeps {sweeps}, timed launches {launches}")
                assert launches == sweeps
                if retried:
                    assert passes > 1 and sweeps > 1, (env, passes)
                assert (chunks > 1) == chunked, (env, chunks)
    finally:
        g.free()


def test_knobs_are_not_in_the_product_build(ctx, records, monkeypatch):
    names, seqs = records
    g = to_device(ctx, names, seqs)
    try:
        monkeypatch.setenv("NTS_MINHASH_IV_BUDGET", "1")
        g.minhash_intervals(_intervals(21, 100), 21, 100)
        assert ctx.minhash_intervals_stats()[1] == 1
    finally:
        g.free()


def test_pair_counts_equal_divergence_distance(ctx):
    rng = np.random.default_rng(9)
    s = 200
    lengths = [200, 200, 200, 150, 37, 1, 0, 0, 200, 200, 64, 65, 200]
    rows = [np.sort(rng.choice(3000, size=n, replace=False)).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15 >> 12) for n in lengths]
    rows[8] = rows[0].copy()                                                   # identical to row 0
    rows[9] = rows[1] + np.uint64(1)                                           # disjoint from everything (odd multiples + 1)
    rows[12] = np.sort(np.concatenate([rows[0][:120], rows[9][:80]]))          # shares a prefix of row 0
    rows = [np.unique(r) for r in rows]
    sk = np.zeros((len(rows), s), dtype=np.uint64)
    cnt = np.array([r.size for r in rows], dtype=np.uint32)
    for i, r in enumerate(rows):
        sk[i, :r.size] = r
    pairs = [(i, j) for i in range(len(rows)) for j in range(len(rows))]      # every ordered pair: random, unequal, empty, identical, disjoint
    shared, size = ctx.minhash_pairs(sk, cnt, [a for a, _ in pairs], [b for _, b in pairs])
    seen = set()
    for (a, b), sh, sz in zip(pairs, shared, size):
        _, sh_ref, sz_ref = divergence.distance(rows[a], rows[b], 21, s)
        assert (int(sh), int(sz)) == (sh_ref, sz_ref), (a, b, int(sh), int(sz), sh_ref, sz_ref)
        seen.add("empty" if sz_ref == 0 else "identical" if sh_ref == sz_ref else "disjoint" if sh_ref == 0 else "partial")
    assert seen == {"empty", "identical", "disjoint", "partial"}
    # a second shape: s = 1 and s larger than a wave's turn
    for s2 in (1, 1000):
        rows2 = [np.unique(rng.integers(0, 5 * s2 + 5, size=rng.integers(0, s2 + 1)).astype(np.uint64)) for _ in range(12)]
        sk2 = np.zeros((12, s2), dtype=np.uint64)
        for i, r in enumerate(rows2):
            sk2[i, :r.size] = r
        pa, pb = rng.integers(0, 12, size=60), rng.integers(0, 12, size=60)
        shared, size = ctx.minhash_pairs(sk2, [r.size for r in rows2], pa, pb)
        for a, b, sh, sz in zip(pa, pb, shared, size):
            assert (int(sh), int(sz)) == divergence.distance(rows2[a], rows2[b], 21, s2)[1:], (s2, a, b)
    assert ctx.minhash_pairs(sk, cnt, [], [])[0].size == 0


def test_distance_follows_the_sequence(ctx):
    """genome B's contig 1 is genome A's with 0.5 % of the bases substituted, its contig 2 with 5 %: every interval on contig 2 is
    further than every interval on contig 1, and each D lies within 4 standard errors of -ln(1 - p) -- the standard error of
    j = shared / size as a binomial share of s draws, carried through dD/dj = -1 / (k j (1 + j))"""
    k, s, ln = 21, 1000, 250_000
    a = synth.make_ancestor(2 * ln, 2, seed=71)
    rates = (0.005, 0.05)
    # derive_genome substitutes each base with probability divergence / 2, always by another base
    b = [synth.derive_genome([a[c]], 2 * rates[c], 1, seed=500 + c, structural=False)[0] for c in range(2)]
    for c in range(2):
        assert abs(float(np.mean(a[c] != b[c])) - rates[c]) <= 5 * math.sqrt(rates[c] * (1 - rates[c]) / ln)
    names = ["c1", "c2"]
    ga = to_device(ctx, names, [x.tobytes() for x in a])
    gb = to_device(ctx, names, [x.tobytes() for x in b])
    try:
        iv = [(c, lo, hi) for c in range(2) for lo, hi in ((0, ln), (0, ln // 2), (ln // 2, ln))]
        ska, na, _ = ga.minhash_intervals(iv, k, s)
        skb, nb, _ = gb.minhash_intervals(iv, k, s)
        n = len(iv)
        shared, size = ctx.minhash_pairs(np.concatenate([ska, skb]), np.concatenate([na, nb]), np.arange(n), np.arange(n) + n)
        dist = []
        for (c, lo, hi), sh, sz in zip(iv, shared, size):
            assert sz == s
            d = divergence.distance_of_counts(sh, sz, k)
            x = (1 - rates[c]) ** k
            j = x / (2 - x)
            se = math.sqrt(j * (1 - j) / s) / (k * j * (1 + j))
            expect = -math.log(1 - rates[c])
            print(f"contig {c + 1} [{lo}, {hi}): D {d:.6f}, expected {expect:.6f}, standard error {se:.6f} (shared {sh}/{sz})")
            assert abs(d - expect) <= 4 * se, (c, lo, hi, d, expect, se)
            dist.append((c, d))
        assert max(d for c, d in dist if c == 0) < min(d for c, d in dist if c == 1)
    finally:
        ga.free()
        gb.free()


def _run(cmd, cwd, env=None, timeout=900):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env or dict(os.environ, PYTHONPATH=ROOT))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_ntsynt_assess_end_to_end(tmp_path):
    paths = synth.make_family(str(tmp_path), 3, 600_000, 2, 0.01, seed=13, micro=6)
    params = ["-d", "1", "-k", "24", "-w", "300", "--w_rounds", "100", "10", "--indel", "500", "--merge", "3000", "-b", "300", "-p", "a"]
    ntsynt = [sys.executable, os.path.join(ROOT, "bin", "ntSynt")]
    plain, with_, many = tmp_path / "plain", tmp_path / "assess", tmp_path / "many"
    for d in (plain, with_, many):
        d.mkdir()
    r = _run(ntsynt + paths + params, plain)
    assert r.returncode == 0, r.stderr[-3000:]
    r = _run(ntsynt + paths + params + ["--assess", "--benchmark"], with_)
    assert r.returncode == 0, r.stderr[-3000:]
    same = ["a.synteny_blocks.tsv", "a.pre-collinear-merge.synteny_blocks.tsv"] + [f"{os.path.basename(p)}.k24.w300.tsv" for p in paths]
    for name in same:
        assert (plain / name).read_bytes() == (with_ / name).read_bytes() and (plain / name).stat().st_size > 0, name
    assert not (plain / "a.block_stats.tsv").exists() and not (plain / "a.block_divergence.tsv").exists()
    assert "assess\t" in (with_ / "a.stage_times.tsv").read_text()
    blocks = assess.read_blocks(str(with_ / "a.synteny_blocks.tsv"))
    per_block = {}
    for row in blocks:
        per_block[row.block_id] = per_block.get(row.block_id, 0) + 1
    n_pairs = sum(n * (n - 1) // 2 for n in per_block.values())
    assert len(per_block) > 3 and n_pairs == 3 * len(per_block)             # every block in all three genomes: blocks x pairs
    lines = (with_ / "a.block_divergence.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(assess.DIVERGENCE_COLUMNS) and lines[-1] == "# k 21, sketch 1000"
    assert len(lines) - 2 == n_pairs
    ids = [int(ln.split("\t")[0]) for ln in lines[1:-1]]
    assert ids == sorted(ids)
    dists = [float(ln.split("\t")[3]) for ln in lines[1:-1]]
    assert 0.0 < float(np.median(dists)) < 0.03                                # (1 % family: about 0.01)
    stats = (with_ / "a.block_stats.tsv").read_text().splitlines()
    assert stats[0].split("\t") == list(assess.STATS_COLUMNS) and int(stats[1].split("\t")[0]) == len(per_block)
    # the tool on the files of that run reproduces both files
    fais = [str(with_ / f"{os.path.basename(p)}.fai") for p in paths]
    r = _run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_block_stats"), "--tsv", str(with_ / "a.synteny_blocks.tsv"), "--fai"] + fais +
             ["--fastas"] + paths + ["--divergence-out", str(tmp_path / "again.tsv")], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.encode() == (with_ / "a.block_stats.tsv").read_bytes()
    assert (tmp_path / "again.tsv").read_bytes() == (with_ / "a.block_divergence.tsv").read_bytes()
    # other sketch parameters are honoured
    r = _run(ntsynt + paths + params + ["--assess", "--assess-k", "16", "--assess-s", "200"], many)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (many / "a.block_divergence.tsv").read_text().splitlines()[-1] == "# k 16, sketch 200"


def test_assess_is_refused_under_two_ranks(tmp_path):
    paths = synth.make_family(str(tmp_path), 2, 200_000, 1, 0.01, seed=14)
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT, NTS_RCCL_LIB=STANDIN, MASTER_ADDR="127.0.0.1", NTS_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "1", "-p", "p", "--assess"]
    r = _run(cmd, out, env=env, timeout=300)
    assert r.returncode != 0
    assert "--assess works from the genomes resident on one GPU" in r.stderr
    assert os.listdir(out) == []

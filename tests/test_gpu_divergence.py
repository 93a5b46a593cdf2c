"""Divergence estimate on the GPU: nts_minhash (k_hash<MODE_MINHASH> + the device set, csrc/nts_minhash.inc) against the CPU reference
sketch and against np.unique(hash_all), both retry directions of the threshold forced, slices merged, Mash distances of 3 Gbp
relatives against the substitution distance of their generator, `ntSynt -d auto` end to end (one rank and two), and
bin/ntsynt_divergence's table."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ntsynt_amd import divergence, synth
from tests.divergence_ref import SENTINEL, ref_sketch
from tests.helpers import random_records, to_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN = os.path.join(ROOT, "tests", "rccl_standin", "librccl_standin.so")


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _unique_sketch(g, k, s):
    h = np.unique(g.hash_all(k))
    return h[h != SENTINEL][:s]


def _sweeps(c, k, s, g):
    "(sketch, number of sweeps it took)"
    c.profile(2)
    try:
        before = c.timing("minhash")[1]
        sk = g.minhash(k, s)
        return sk, c.timing("minhash")[1] - before
    finally:
        c.profile(False)


@pytest.fixture(scope="module")
def random_genome():
    rng = np.random.default_rng(21)
    seqs = random_records(rng, [200_000, 50_000, 15, 3_000, 0, 120_000, 140, 64_000], n_frac=0.03, lower_frac=0.1)
    return [f"r{i}" for i in range(len(seqs))], seqs


@pytest.mark.parametrize("k", [16, 21, 24, 32, 100, 150])
def test_minhash_equals_the_cpu_reference(ctx, random_genome, k):
    names, seqs = random_genome
    g = to_device(ctx, names, seqs)
    try:
        full = _unique_sketch(g, k, 10**9)
        for s in (1, 1000, 10000):
            got = g.minhash(k, s)
            assert got.dtype == np.uint64 and got.size == min(s, full.size)
            assert np.array_equal(got, ref_sketch(seqs, k, s)), (k, s)
            assert np.array_equal(got, full[:s]), (k, s)
    finally:
        g.free()


def test_fewer_distinct_kmers_than_s(ctx):
    seqs = [b"ACGTTGC" * 3000, b"acgttgcNNNNACGTTGCACGTTGCACGTTGCACG", b"ACG", random_records(np.random.default_rng(2), [2000])[0]]
    g = to_device(ctx, ["a", "b", "c", "d"], seqs)
    try:
        for k in (21, 150):
            ref = ref_sketch(seqs, k, 10000)
            assert 0 < ref.size < 10000
            assert np.array_equal(g.minhash(k, 10000), ref)
    finally:
        g.free()
    empty = to_device(ctx, ["x"], [b"ACGTNNNNACGT"])
    try:
        assert empty.minhash(21, 100).size == 0
    finally:
        empty.free()


def test_forced_thresholds_and_capacity_give_the_same_sketch(ctx_x, random_genome, monkeypatch):
    names, seqs = random_genome
    g = to_device(ctx_x, names, seqs)
    try:
        for k, s in ((21, 1000), (24, 1), (150, 300)):
            ref = ref_sketch(seqs, k, s)
            _, n0 = _sweeps(ctx_x, k, s, g)
            assert n0 == 1 or s == 1                            # the common case: one sweep (s = 1: ~4 expected survivors, may be 0)
            for env, retried in (({"NTS_MINHASH_TAU0": "1"}, True),                          # far too low: raised
                                 ({"NTS_MINHASH_TAU0": str(2**64 - 1)}, False),              # everything survives, fits 2^22
                                 ({"NTS_MINHASH_TAU0": str(2**64 - 1), "NTS_MINHASH_CAP": "16"}, True),  # overflows: lowered
                                 ({"NTS_MINHASH_CAP": "1"}, None),                           # clamped to 4 s
                                 ({"NTS_MINHASH_TAU0": str(2**40), "NTS_MINHASH_CAP": "64"}, True)):
                for key, val in env.items():
                    monkeypatch.setenv(key, val)
                got, n = _sweeps(ctx_x, k, s, g)
                for key in env:
                    monkeypatch.delenv(key)
                assert np.array_equal(got, ref), (k, s, env)
                if retried is not None:
                    assert (n > 1) == retried, (k, s, env, n)
    finally:
        g.free()


def test_knobs_are_not_in_the_product_build(ctx, random_genome, monkeypatch):
    names, seqs = random_genome
    g = to_device(ctx, names, seqs)
    try:
        monkeypatch.setenv("NTS_MINHASH_TAU0", "1")
        _, n = _sweeps(ctx, 21, 1000, g)
        assert n == 1
    finally:
        g.free()


def test_sketches_of_slices_merge_into_the_whole(ctx, random_genome):
    names, seqs = random_genome
    g = to_device(ctx, names, seqs)
    try:
        for k, s in ((21, 10000), (32, 500)):
            whole = g.minhash(k, s)
            cuts = [0, 1, 4, 6, len(names)]
            acc = np.zeros(0, np.uint64)
            for a, b in zip(cuts[:-1], cuts[1:]):
                part = g.slice(a, b)
                try:
                    acc = divergence.merge(acc, part.minhash(k, s), s)
                finally:
                    part.free()
            assert np.array_equal(acc, whole)
    finally:
        g.free()


def test_assembly_like_genome(ctx):
    """~200 Mbp with satellite arrays, interspersed repeat families, segmental duplications, a tail of short scaffolds and N gaps: the
    sketch equals np.unique over every k-mer's hash"""
    from ntsynt_amd.device import Genome
    plan = synth.realistic_plan(4, 50_000_000, 1, seed=29, n_scaffolds=40, n_tail=200, n_gaps=60, sat_scale=0.5)
    g = Genome.synth_plan(ctx, plan, 29, 1001, 0.0065, rep=synth.REPEATS, names=plan[2])
    try:
        assert g.total_bp > 190_000_000
        h = np.unique(g.hash_all(21))
        h = h[h != SENTINEL]
        for s in (1, 10000):
            got, n = _sweeps(ctx, 21, s, g)
            assert np.array_equal(got, h[:s]), s
            print(f"assembly-like {g.total_bp} bp, k 21, s {s}: {n} sweep(s)")
    finally:
        g.free()


def _rate_for(p):
    "per-genome substitution rate r of Genome.synth whose relatives differ at p: p = 2r(1 - r) + (2/3) r^2"
    return (2.0 - math.sqrt(4.0 - 16.0 / 3.0 * p)) / (8.0 / 3.0)


@pytest.mark.parametrize("p", [0.001, 0.01, 0.1])
def test_mash_distance_of_3gbp_relatives(ctx, p):
    """two 3 Gbp relatives (every base substituted with probability r in each, independently): D within 3-4 binomial standard
    errors of j at s = 10^4 of -ln(1 - p).  p is confirmed on 20 Mbp of the generated bases"""
    from ntsynt_amd.device import Genome
    r = _rate_for(p)
    sk = []
    sample = []
    for j in range(2):
        g = Genome.synth(ctx, 3_000_000_000, 24, 77, 100 + j, r)
        try:
            sample.append(g.download(1_000_000_000, 20_000_000))
            s_, n = _sweeps(ctx, 21, 10000, g)
            sk.append(s_)
            print(f"3 Gbp p {p}: {n} sweep(s)")
        finally:
            g.free()
    p_gen = float(np.mean(sample[0] != sample[1]))
    assert abs(p_gen - p) <= 5 * math.sqrt(p * (1 - p) / sample[0].size) + 1e-9, (p_gen, p)
    d, shared, size = divergence.distance(sk[0], sk[1], 21, 10000)
    expect = -math.log(1 - p)
    print(f"p {p}: D {d:.6f} vs {expect:.6f} (shared {shared}/{size})")
    assert size == 10000 and abs(d - expect) <= 0.05 * expect + 2e-4, (d, expect)


def _family(tmp_path):
    # structural=False: the structural events would add unshared sequence; without them p = the substitution distance alone
    paths = synth.make_family(str(tmp_path), 3, 2_000_000, 3, 0.03, seed=61, structural=False)
    # make_family substitutes each base with probability 0.03 / 2 per genome: pairwise p = 2q(1 - q) + (2/3) q^2
    q = 0.015
    return paths, -math.log(1 - (2 * q * (1 - q) + 2 * q * q / 3))


def _ntsynt(args, cwd, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "ntSynt")] + args, cwd=cwd, capture_output=True, text=True, timeout=900,
                       env=env or dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_ntsynt_auto_end_to_end(tmp_path):
    paths, expect = _family(tmp_path)
    (tmp_path / "auto").mkdir()
    (tmp_path / "num").mkdir()
    out = _ntsynt(paths + ["-d", "auto", "-p", "a"], tmp_path / "auto")
    first = out.splitlines()[0]
    assert first.startswith("Estimated percent divergence: ") and first.endswith("; k 21, sketch 10000)"), first
    printed = first.split()[3]
    d = float(printed) / 100
    assert abs(d - expect) <= 0.05 * expect + 2e-4 + 1e-5, (d, expect)        # (+ the rounding up to 0.001 %)
    assert "\t--block_size 1000\n" in out and "\t--w_rounds [250, 100]\n" in out    # the 1-10 % row
    out_n = _ntsynt(paths + ["-d", printed, "-p", "a"], tmp_path / "num")
    assert out.split("\n", 1)[1] == out_n
    blocks = (tmp_path / "auto" / "a.synteny_blocks.tsv").read_bytes()
    assert blocks and blocks == (tmp_path / "num" / "a.synteny_blocks.tsv").read_bytes()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_ntsynt_auto_two_ranks_match_one(tmp_path):
    assert os.path.exists(STANDIN), "tests/rccl_standin/librccl_standin.so is not built (__graft_entry__.build())"
    paths, _ = _family(tmp_path)
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir()
    many.mkdir()
    out1 = _ntsynt(paths + ["-d", "auto", "-p", "p"], one)
    env = dict(os.environ, PYTHONPATH=ROOT, NTS_RCCL_LIB=STANDIN, MASTER_ADDR="127.0.0.1", NTS_DIST_BACKEND="gloo", NTS_COMM_PIECE="262144")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bin", "ntSynt")] + paths + ["-d", "auto", "-p", "p"]
    r = subprocess.run(cmd, cwd=many, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    est = [ln for ln in r.stdout.splitlines() if ln.startswith("Estimated percent divergence")]
    assert est == [out1.splitlines()[0]]                                 # rank 0 talks; every rank made the same estimate
    for name in ("p.synteny_blocks.tsv", "p.pre-collinear-merge.synteny_blocks.tsv"):
        assert (one / name).read_bytes() == (many / name).read_bytes(), name


def test_divergence_launcher_table(ctx, tmp_path):
    paths, _ = _family(tmp_path)
    out = tmp_path / "d.tsv"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_divergence")] + paths + ["-o", str(out)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = out.read_text().splitlines()
    assert lines[0].split("\t") == ["genome_a", "genome_b", "distance", "shared_hashes", "sketch_size"]
    sk = _sketches(ctx, paths, 21, 10000)
    rows = [ln.split("\t") for ln in lines[1:-1]]
    assert [(a, b) for a, b, *_ in rows] == [(paths[0], paths[1]), (paths[0], paths[2]), (paths[1], paths[2])]
    d_max = 0.0
    for (a, b, d, shared, size), (i, j) in zip(rows, ((0, 1), (0, 2), (1, 2))):
        d_ref, shared_ref, size_ref = divergence.distance(sk[i], sk[j], 21, 10000)
        assert d == f"{d_ref:.6g}" and (int(shared), int(size)) == (shared_ref, size_ref)   # (six significant digits, as Mash prints)
        d_max = max(d_max, d_ref)
    assert lines[-1] == f"# ntSynt -d {divergence.suggested_divergence(d_max)}"
    # -k / -s are honoured
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "ntsynt_divergence"), "-k", "16", "-s", "500"] + paths[:2], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    row = r.stdout.splitlines()[1].split("\t")
    sk16 = _sketches(ctx, paths[:2], 16, 500)
    _, shared_ref, size_ref = divergence.distance(sk16[0], sk16[1], 16, 500)
    assert (int(row[3]), int(row[4])) == (shared_ref, size_ref) and size_ref == 500


def _sketches(ctx, paths, k, s):
    from ntsynt_amd.fasta import read_fasta_device
    out = []
    for p in paths:
        g, _ = read_fasta_device(ctx, p)
        out.append(g.minhash(k, s))
        g.free()
    return out

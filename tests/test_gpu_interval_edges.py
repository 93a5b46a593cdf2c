"""The interval sweeps at the edges of the tile sweep (csrc/nts_tile_sweep.inc): k = 127, 128 and 129 -- the staging area at its fullest
and the switch from staged bases to per-lane loads --, every alignment pos % 16 of a full tile, of the tile cut and of partial lanes,
and intervals that end or begin on a record's seam with another record's valid bases behind it.  All five entry points
(bf_count_intervals, bf_sample_intervals, hset_sample_intervals, minhash_intervals, valid_bases) get the same intervals in one call
per k and are compared with the oracle's statements (tests/helpers.py) by exact equality; the outputs are then checked against one
another, so that an oracle sharing a mistake with a kernel does not pass.  k = 1 and 2 go through the same intervals.  Every test runs
under a time limit of its own (a hung call ends the process, with a traceback).

edge_inputs(), edge_intervals() and the conditions that keep a match from being vacuous need no GPU:
tests/test_interval_edges_oracle_inputs.py checks them on the CPU."""
import faulthandler

import numpy as np
import pytest

from ntsynt_amd import synth
from oracle import nts_oracle as O
from tests.helpers import (END_CASE_KMERS, U64_MAX, genome_end_case, oracle_counts, oracle_sample, oracle_set_sample, oracle_sketches,
                           random_records, to_device)

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
KS = [127, 128, 129]              # FAST_K_MAX - 1, FAST_K_MAX (the fullest staging area), the first k whose lanes read memory
SMALL_KS = [1, 2]
RATES = (1, 3, 16)
SET_RATES = (1, 16)
SKETCH_S = (16, 1024)
SUBSTITUTIONS = 0.02              # synth.derive_genome's pairwise figure: 1 % of the bases of the copy differ (0.99^128 = 28 % of the 128-mers survive)
A, B, C, D = 0, 1, 2, 3
LENGTHS = (45_000, 12_000, 9, 12_000)
N_RUN = (2_000, 2_040)            # D's only N run: inside the record, and the 8193 k-mers that end on D's last base lie behind it
FILTER_BYTES = 86_400             # 691 200 bits for the 69 000 k-mers of the copy: ten bits per k-mer
FULL_TILE = (8191, 8192, 8193)
PARTIAL = (1, 7, 8, 9, 31, 33, 8161)
SEAM = (1, 33, 8191, 8192, 8193)
N_FULL = 16 * len(FULL_TILE)      # the intervals of group 1 come first: 3 r + j is start 1000 + r with FULL_TILE[j] k-mers
SEED = 1160


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


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def edge_inputs():
    """(names, records, a mutated copy's records).  A: 45 kbp without N; B: 12 kbp, follows A directly and begins with valid bases;
    C: 9 bases; D: 12 kbp with one N run of 40, ends the genome.  Lower case here and there, no other N."""
    rng = np.random.default_rng(SEED)
    a, b, c, d = random_records(rng, list(LENGTHS), n_frac=0.0, lower_frac=0.1)
    d = bytearray(d)
    d[N_RUN[0]:N_RUN[1]] = b"N" * (N_RUN[1] - N_RUN[0])
    seqs = [a, b, c, bytes(d)]
    assert all(x in b"ACGTacgt" for x in b[:200]) and seqs[D].upper().count(b"N") == N_RUN[1] - N_RUN[0]
    copy = synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=SEED + 1, structural=False)
    return ["A", "B", "C", "D"], seqs, [c.tobytes() for c in copy]


def edge_intervals(k):
    "(intervals, the k-mers each is meant to hold): one list per k, every entry point gets all of it in one call"
    la, lb, lc, ld = LENGTHS
    rows = []
    # 1. every alignment of a full tile: sixteen consecutive starts take every pos % 16, whatever the record's offset in the code array
    for r in range(16):
        rows += [((A, 1000 + r, 1000 + r + n + k - 1), n) for n in FULL_TILE]
    # 2. every alignment of the tile cut: two full tiles and a tail of five k-mers, one partial lane
    n = 2 * 8192 + 5
    rows += [((A, 11_000 + r, 11_000 + r + n + k - 1), n) for r in range(16)]
    # 3. partial lanes at every alignment: a lane that stops inside, at and just behind a batch of eight; around a lane's 32; 255 full
    #    lanes and a lane of one k-mer
    for r in range(16):
        rows += [((A, 30_000 + r, 30_000 + r + n + k - 1), n) for n in PARTIAL]
    # 4. record seams with live neighbours: up to A's last base (B's bases follow), from B's first base (A's lie before), up to D's
    #    last base (the genome's end); a record shorter than k; an end far beyond the record
    rows += [((A, la - (n + k - 1), la), n) for n in SEAM]
    rows += [((B, 0, n + k - 1), n) for n in SEAM]
    rows += [((D, ld - (n + k - 1), ld), n) for n in SEAM]
    rows += [((C, 0, lc), max(lc - k + 1, 0)), ((B, 0, 10**12), lb - k + 1)]
    # 5. across D's N run, up to the base before it, from the base behind it
    rows += [((D, N_RUN[0] - 300, N_RUN[1] + 300), 2 * (300 - k + 1)),
             ((D, N_RUN[0] - 700, N_RUN[0]), 700 - k + 1),
             ((D, N_RUN[1], N_RUN[1] + 700), 700 - k + 1)]
    assert ld - (max(SEAM) + k - 1) >= N_RUN[1] and 30_000 + 15 + max(PARTIAL) + k - 1 <= la and 11_000 + 15 + 2 * 8192 + 5 + k - 1 <= 30_000
    return [r[0] for r in rows], [r[1] for r in rows]


def base_runs(seq, start, end):
    "the lengths of the runs of A/C/G/T (either case) in seq[start:end], clipped to the record: no hashing, no oracle"
    seg = np.frombuffer(seq[min(start, len(seq)):max(min(end, len(seq)), min(start, len(seq)))], dtype=np.uint8)
    ok = np.isin(seg, np.frombuffer(b"ACGTacgt", dtype=np.uint8)).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], ok, [0]))))
    return [int(b - a) for a, b in zip(edges[::2], edges[1::2])]


def set_members(copy, k):
    "the hashes of the copy's k-mers under the rate-16 threshold -- what a gap sampling at that rate collects --, and the two ends of the range"
    h = np.concatenate([O.hash_all(s, k)[1] for s in copy])
    return np.concatenate([h[h <= np.uint64(U64_MAX // 16)], np.array([0, U64_MAX], dtype=np.uint64)])


def last_lane(k, per_rec, bits_held, iv):
    "(held, held and not sampled at rate 16) among the last 32 k-mers of an interval that is one piece"
    rec, start, end = iv
    pos, h0 = per_rec[rec]
    at = np.flatnonzero((pos >= end - k - 31) & (pos + k <= end) & (pos >= start))
    held = bits_held[rec][at]
    return int(held.sum()), int((held & (h0[at] > np.uint64(U64_MAX // 16))).sum())


class Case:
    "one k: inputs, the oracle's hashes, the device objects, and every entry point's output over the whole list -- computed once"

    def __init__(self, ctx, k):
        from ntsynt_amd.device import BloomFilter, HashSet
        self.k = k
        self.names, self.seqs, self.copy = edge_inputs()
        self.iv, self.want_kmers = edge_intervals(k)
        self.bits = O.bf_build(O.Genome(self.names, self.copy), k, FILTER_BYTES)
        self.ones_bits = np.full(FILTER_BYTES, 0xFF, dtype=np.uint8)
        self.per_rec = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in self.seqs)]
        self.members = set_members(self.copy, k)
        self.g = to_device(ctx, self.names, self.seqs)
        self.bf = BloomFilter(ctx, FILTER_BYTES, k)
        gc = to_device(ctx, self.names, self.copy)
        try:
            self.bf.insert(gc)
        finally:
            gc.free()
        self.ones = BloomFilter(ctx, FILTER_BYTES, k, ones=True)
        self.hs = HashSet(ctx, self.members)
        self._out = {}

    def run(self, iv):
        "the five entry points, the filter of ones included, over `iv` in one call each"
        g, k = self.g, self.k
        out = {"count": g.bf_count_intervals(self.bf, iv, k), "ones_count": g.bf_count_intervals(self.ones, iv, k), "valid": g.valid_bases(iv),
               "ones_sample": g.bf_sample_intervals(self.ones, iv, k, 1)}
        for rate in RATES:
            out["sample", rate] = g.bf_sample_intervals(self.bf, iv, k, rate)
        for rate in SET_RATES:
            out["set", rate] = g.hset_sample_intervals(self.hs, iv, k, rate)
        for s in SKETCH_S:
            out["sketch", s] = g.minhash_intervals(iv, k, s)
        return out

    def out(self):
        if not self._out:
            self._out = self.run(self.iv)
        return self._out

    def free(self):
        for x in (self.g, self.bf, self.ones, self.hs):
            x.free()


@pytest.fixture(scope="module", params=KS + SMALL_KS)
def case(ctx, request):
    c = Case(ctx, request.param)
    yield c
    c.free()


def by_interval(recs, counts):
    "the records of a sampling call, interval by interval"
    assert int(counts.sum()) == recs.size
    return np.split(recs, np.cumsum(counts.astype(np.int64))[:-1])


def same_but_iv(x, y):
    "two record arrays agree once `iv` is set aside"
    return np.array_equal(x["h0"], y["h0"]) and np.array_equal(x["off"], y["off"])


def check_records(what, k, iv, got, exp):
    "a sampling call against the oracle: counts, then order, h0, iv and off of every record; the rows of the intervals that differ"
    (recs, counts), (exp_recs, exp_counts) = got, exp
    from ntsynt_amd.device import SAMPLE_DTYPE
    assert recs.dtype == SAMPLE_DTYPE and counts.dtype == np.uint64 and counts.shape == (len(iv),)
    print(f"k {k} {what}: {recs.size} records, oracle {exp_recs.size}")
    for i in np.flatnonzero(counts != exp_counts):
        print(f"k {k} {what} {iv[i]}: {int(counts[i])} records, oracle {int(exp_counts[i])}")
    assert np.array_equal(counts, exp_counts), (k, what)
    for i, (x, y) in enumerate(zip(by_interval(recs, counts), by_interval(exp_recs, exp_counts))):
        if not np.array_equal(x, y):
            j = int(np.flatnonzero(x != y)[0])
            print(f"k {k} {what} {iv[i]}: record {j} of {x.size} is {x[j]}, oracle {y[j]}")
    assert np.array_equal(recs, exp_recs), (k, what)


# ---- 1. each entry point against the oracle ---------------------------------------------------------------------------------------------
def test_the_filter_is_the_oracles(case):
    "the conditions checked on the CPU hold for the bits the GPU probes"
    assert np.array_equal(case.bf.to_numpy(), case.bits), case.k
    assert np.array_equal(case.ones.to_numpy(), case.ones_bits), case.k


def test_counts_and_valid_bases_equal_the_oracle(case):
    k, iv, seqs = case.k, case.iv, case.seqs
    kmers, hits = case.out()["count"]
    valid = case.out()["valid"]
    assert kmers.dtype == np.uint64 and hits.dtype == np.uint64 and kmers.shape == hits.shape == (len(iv),)
    ref = oracle_counts(seqs, k, case.bits, iv)
    for i, row in enumerate(iv):
        print(f"k {k} {row}: kmers {int(kmers[i])} hits {int(hits[i])} oracle {ref[i]} valid bases {int(valid[i])}")
    for i, row in enumerate(iv):
        assert (int(kmers[i]), int(hits[i])) == ref[i], (k, row, int(kmers[i]), int(hits[i]), ref[i])
    assert [int(x) for x in kmers] == case.want_kmers, k                         # the intervals are what they are for
    total_k, total_h = sum(r[0] for r in ref), sum(r[1] for r in ref)
    if k in KS:
        assert 0 < total_h < total_k, (k, total_h, total_k)                      # never a vacuous match
    else:
        assert 0 < total_h == total_k, (k, total_h, total_k)                     # the copy holds each of the 2 (10) canonical 1-mers (2-mers): no seed gives a miss
    # valid bases and k-mers from the runs of bases alone: valid - (k - 1) x pieces where every run is a piece
    for (rec, start, end), v, n in zip(iv, valid, kmers):
        runs = base_runs(seqs[rec], start, end)
        assert int(v) == sum(runs), (k, rec, start, end)
        assert int(n) == sum(max(ln - k + 1, 0) for ln in runs), (k, rec, start, end)
        if runs and min(runs) >= k:
            assert int(n) == int(v) - (k - 1) * len(runs), (k, rec, start, end)
    assert sum(len(base_runs(seqs[rec], start, end)) == 1 for rec, start, end in iv) == len(iv) - 1      # all but the one across the N run


def test_every_full_tile_has_live_kmers_in_its_last_lane(case):
    """a wrong last word of staging must not hide: among the last 32 k-mers of every interval of group 1 the filter holds one, and
    holds one that a sample at rate 16 leaves out -- by the oracle, which the counts of the kernels are compared with elsewhere"""
    k = case.k
    held = [np.array([O.bf_contains(case.bits, h) for h in h0], dtype=bool) for _, h0 in case.per_rec]
    for row in case.iv[:N_FULL]:
        n_held, n_unsampled = last_lane(k, case.per_rec, held, row)
        assert n_held > 0 and n_unsampled > 0, (k, row, n_held, n_unsampled)


def test_samples_equal_the_oracle(case):
    k, iv = case.k, case.iv
    kmers, hits = case.out()["count"]
    sizes = {}
    for rate in RATES:
        got = case.out()["sample", rate]
        check_records(f"rate {rate}", k, iv, got, oracle_sample(case.seqs, k, case.bits, iv, rate))
        sizes[rate] = got[0].size
    assert np.array_equal(case.out()["sample", 1][1], hits), k                   # at rate 1 the sample counts what the counting kernel counts
    if k in KS:
        assert 0 < sizes[16] < sizes[3] < sizes[1] < int(kmers.sum()), (k, sizes)
    else:                                                                        # the 2 (10) hashes are constants of the hash function: none lies under 2^64 / 16
        assert 0 == sizes[16] <= sizes[3] <= sizes[1] == int(kmers.sum()), (k, sizes)
    # group 1 nests: the records of 8191 k-mers from a start are the first of those of 8192, and those the first of 8193
    recs, counts = case.out()["sample", 1]
    parts = by_interval(recs, counts)
    for r in range(16):
        a, b, c = (parts[3 * r + j] for j in range(3))
        assert a.size <= b.size <= c.size and same_but_iv(a, b[:a.size]) and same_but_iv(b, c[:b.size]), (k, r)


def test_set_sweep_equals_the_oracle(case):
    k, iv = case.k, case.iv
    kmers = case.out()["count"][0]
    for rate in SET_RATES:
        got = case.out()["set", rate]
        check_records(f"set, rate {rate}", k, iv, got, oracle_set_sample(case.per_rec, case.seqs, k, case.members, iv, rate))
        if k in KS:
            assert 0 < got[0].size < int(kmers.sum()), (k, rate)                 # never a vacuous match
    # every member lies under the rate-16 threshold but 2^64 - 1, which no k-mer here hashes to: the two rates give the same records
    assert np.array_equal(case.out()["set", 1][0], case.out()["set", 16][0]), k
    if k not in KS:                                                              # the members are 0 and 2^64 - 1 alone: a k-mer that is skipped must not pass for 0
        assert case.out()["set", 1][0].size == 0 < int(kmers.sum()), k


def test_sketches_equal_the_oracle(case):
    k, iv = case.k, case.iv
    for s in SKETCH_S:
        out, counts, n_kmers = case.out()["sketch", s]
        ref, ref_nk = oracle_sketches(case.seqs, k, s, iv)
        assert out.shape == (len(iv), s) and counts.dtype == np.uint32 and n_kmers.dtype == np.uint64
        for i, row in enumerate(iv):
            assert int(n_kmers[i]) == ref_nk[i], (k, s, row, int(n_kmers[i]), ref_nk[i])
            assert int(counts[i]) == ref[i].size, (k, s, row, int(counts[i]), ref[i].size)
            assert np.array_equal(out[i, :counts[i]], ref[i]), (k, s, row)
        if k in KS:
            assert [int(c) for c in counts] == [min(s, n) for n in case.want_kmers], (k, s)     # random sequence: no repeated k-mer


# ---- 2. the outputs against one another -------------------------------------------------------------------------------------------------
def test_a_filter_of_ones_gives_every_kmer(case):
    "every k-mer of every interval, hash by hash: counts, the rate-1 records against the oracle, the sketches from the records"
    k, iv = case.k, case.iv
    kmers, hits = case.out()["ones_count"]
    recs, counts = case.out()["ones_sample"]
    assert np.array_equal(kmers, hits) and np.array_equal(counts, kmers) and np.array_equal(kmers, case.out()["count"][0]), k
    assert [int(x) for x in counts] == case.want_kmers, k
    check_records("ones, rate 1", k, iv, (recs, counts), oracle_sample(case.seqs, k, case.ones_bits, iv, 1))
    parts = by_interval(recs, counts)
    for s in SKETCH_S:
        out, n_sk, _ = case.out()["sketch", s]
        for i, row in enumerate(iv):
            h = np.unique(parts[i]["h0"])
            assert np.array_equal(h[h != np.uint64(U64_MAX)][:s], out[i, :n_sk[i]]), (k, s, row)


def test_reversed_list_gives_the_same_per_interval(case):
    k, iv = case.k, case.iv
    n = len(iv)
    fwd, rev = case.out(), case.run(iv[::-1])
    for key in ("count", "ones_count"):
        assert all(np.array_equal(a, b[::-1]) for a, b in zip(fwd[key], rev[key])), (k, key)
    assert np.array_equal(fwd["valid"], rev["valid"][::-1]), k
    for key in [("sample", r) for r in RATES] + [("set", r) for r in SET_RATES] + ["ones_sample"]:
        (recs, counts), (rrecs, rcounts) = fwd[key], rev[key]
        assert np.array_equal(counts, rcounts[::-1]), (k, key)
        back = np.concatenate(by_interval(rrecs, rcounts)[::-1])
        assert np.array_equal(back["iv"], n - 1 - recs["iv"].astype(np.int64)), (k, key)
        assert same_but_iv(back, recs), (k, key)
    for s in SKETCH_S:
        assert all(np.array_equal(a, b[::-1]) for a, b in zip(fwd["sketch", s], rev["sketch", s])), (k, s)


# ---- 3. the end of the genome at the staging limit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "tests/helpers.py's genome_end_case, which the sibling modules run at k = 24 and 150, through all five entry points"
    from ntsynt_amd.device import BloomFilter, HashSet
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], SUBSTITUTIONS, 1, seed=79, structural=False)]
    bits = O.bf_build(O.Genome(names, copy), k, 1 << 16)
    per_rec = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in seqs)]
    members = set_members(copy, k)
    g, gc = to_device(ctx, names, seqs), to_device(ctx, names, copy)
    bf = BloomFilter(ctx, 1 << 16, k)
    hs = HashSet(ctx, members)
    try:
        bf.insert(gc)
        assert np.array_equal(bf.to_numpy(), bits), k
        kmers, hits = g.bf_count_intervals(bf, iv, k)
        ref = oracle_counts(seqs, k, bits, iv)
        for i, row in enumerate(iv):
            print(f"k {k} {row}: kmers {int(kmers[i])} hits {int(hits[i])} oracle {ref[i]}")
        assert [r[0] for r in ref[:12]] == list(END_CASE_KMERS) * 2 and ref[12][0] == 500 - k + 1 + 460 - k + 1, ref
        assert [(int(a), int(b)) for a, b in zip(kmers, hits)] == ref
        assert 0 < sum(r[1] for r in ref) < sum(r[0] for r in ref)               # never a vacuous match
        for rate in RATES:
            got = g.bf_sample_intervals(bf, iv, k, rate)
            check_records(f"genome end, rate {rate}", k, iv, got, oracle_sample(seqs, k, bits, iv, rate))
            assert 0 < got[0].size < int(kmers.sum()), (k, rate)                   # never a vacuous match
            if rate == 1:
                assert np.array_equal(got[1], hits), k
        for rate in SET_RATES:
            got = g.hset_sample_intervals(hs, iv, k, rate)
            check_records(f"genome end, set, rate {rate}", k, iv, got, oracle_set_sample(per_rec, seqs, k, members, iv, rate))
            assert 0 < got[0].size < int(kmers.sum()), (k, rate)
        for s in SKETCH_S:
            out, counts, n_kmers = g.minhash_intervals(iv, k, s)
            sk, nk = oracle_sketches(seqs, k, s, iv)
            assert [int(x) for x in n_kmers] == nk and [int(c) for c in counts] == [min(s, n) for n in nk], (k, s)
            assert all(np.array_equal(out[i, :counts[i]], sk[i]) for i in range(len(iv))), (k, s)
        valid = g.valid_bases(iv)
        assert [int(v) for v in valid] == [sum(base_runs(seqs[rec], start, end)) for rec, start, end in iv], k
        assert [int(v) - (k - 1) for v in valid[:12]] == list(END_CASE_KMERS) * 2, k
    finally:
        for x in (g, gc, bf, hs):
            x.free()

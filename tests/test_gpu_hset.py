"""The exact hash set on the GPU (csrc/nts_hset.inc): nts_hset_contains against a Python set on the sizes and keys at which an open-addressed
table can go wrong; nts_hset_sample_intervals against the oracle -- O.hash_all of the record, the threshold, membership in the set by
np.isin -- record for record on tests/test_gpu_gap_links.py's inputs and intervals; partial lanes up to the genome's last base; the
launch cut forced on the experiments build; the errors.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from ntsynt_amd import synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.helpers import END_CASE_KMERS, genome_end_case, to_device
from tests.helpers import oracle_set_sample as oracle_sample

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
U64_MAX = (1 << 64) - 1
TIMERS = ("hset_sample_count", "hset_sample_write")


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


# ---- 1. the set alone -----------------------------------------------------------------------------------------------------------------
def check_set(ctx, keys, queries, what):
    "build the set of `keys`, ask for `queries`, compare with a Python set"
    from ntsynt_amd.device import HashSet
    keys, queries = np.asarray(keys, dtype=np.uint64), np.asarray(queries, dtype=np.uint64)
    members = set(int(x) for x in keys)
    exp = np.array([int(q) in members for q in queries], dtype=bool)
    hs = HashSet(ctx, keys)
    try:
        got = hs.contains(queries)
    finally:
        hs.free()
    print(f"{what}: {keys.size} keys ({len(members)} distinct), {queries.size} queries, {int(exp.sum())} members among them")
    assert got.dtype == bool and got.shape == exp.shape, what
    assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:10])
    return got


def test_sizes_around_a_power_of_two(ctx):
    rng = np.random.default_rng(411)
    m = 10
    for n in (0, 1, 2**m - 1, 2**m, 2**m + 1):
        keys = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
        others = rng.integers(0, U64_MAX, size=max(n, 8), dtype=np.uint64, endpoint=True)
        got = check_set(ctx, keys, np.concatenate([keys, others, np.array([0, U64_MAX], dtype=np.uint64)]), f"n = {n}")
        assert int(got[:n].sum()) == n and not got[n:].any()                     # (a random 64-bit value is not among 1025 others)


def test_zero_and_all_ones_present_and_absent(ctx):
    rng = np.random.default_rng(412)
    some = rng.integers(1, U64_MAX, size=300, dtype=np.uint64)                  # neither 0 nor 2^64 - 1
    ends = np.array([0, U64_MAX, 1, U64_MAX - 1], dtype=np.uint64)
    for with_zero in (False, True):
        for with_max in (False, True):
            keys = np.concatenate([some, np.array([0] * with_zero + [U64_MAX] * with_max, dtype=np.uint64)])
            got = check_set(ctx, keys, np.concatenate([ends, some]), f"0 {'in' if with_zero else 'out'}, 2^64 - 1 {'in' if with_max else 'out'}")
            assert [bool(x) for x in got[:4]] == [with_zero, with_max, False, False]
    check_set(ctx, [U64_MAX], ends, "2^64 - 1 alone")
    check_set(ctx, [0], ends, "0 alone")
    check_set(ctx, [U64_MAX, U64_MAX, 0, 0], ends, "both, twice")


def test_keys_that_differ_in_few_bits_or_lie_under_a_threshold(ctx):
    rng = np.random.default_rng(413)
    i = np.arange(4096, dtype=np.uint64)
    base = np.uint64(0x0005A5A5A5A5A000)                                        # low 12 and top 12 bits clear
    low = base | i
    top = base | (i << np.uint64(52))
    under = rng.integers(0, U64_MAX >> 20, size=4096, dtype=np.uint64, endpoint=True)
    assert np.unique(low >> np.uint64(12)).size == 1 and np.unique(top & np.uint64((1 << 52) - 1)).size == 1 and int(under.max()) <= U64_MAX >> 20
    for what, keys in (("low 12 bits", low), ("top 12 bits", top), ("under 2^44", under)):
        half = keys[::2]                                                       # every other one is a member; the rest are near misses
        got = check_set(ctx, half, np.concatenate([keys, keys ^ np.uint64(1 << 30)]), what)
        assert int(got.sum()) == np.unique(half).size


def test_random_keys_with_duplicates(ctx):
    rng = np.random.default_rng(414)
    n = 200_000
    keys = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
    dup = rng.choice(n, size=n * 3 // 100, replace=False)
    keys[dup] = keys[(dup + 1) % n]                                            # 3 % of them repeat a neighbour
    assert 0.025 < 1 - np.unique(keys).size / n < 0.035
    others = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
    got = check_set(ctx, keys, np.concatenate([keys, others]), "2e5 random keys")
    assert got[:n].all() and not got[n:].any()


# ---- 2. the sweep ---------------------------------------------------------------------------------------------------------------------
_hashes = {}


def kmers_of(tag, seqs, k):
    "per record (positions, hashes) by the oracle, once per input and k"
    if (tag, k) not in _hashes:
        _hashes[(tag, k)] = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in seqs)]
    return _hashes[(tag, k)]


def set_of_copy(tag, copy, k, rate):
    "the hashes of the mutated copy under the rate's threshold: what a gap sampling at that rate would have collected"
    h = np.concatenate([h for _, h in kmers_of(tag, copy, k)])
    return h[h <= np.uint64(U64_MAX // rate)]


def inside_counts(per_rec, seqs, k, intervals):
    out = []
    for rec, start, end in intervals:
        pos, _ = per_rec[rec]
        out.append(int(((pos >= min(start, len(seqs[rec]))) & (pos + k <= min(end, len(seqs[rec])))).sum()))
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("k", KS)
def test_sweep_equals_the_oracle(ctx, k):
    from ntsynt_amd.device import SAMPLE_DTYPE, HashSet
    names, seqs, copy = L.sample_inputs()
    per_rec = kmers_of("seqs", seqs, k)
    iv = L.sample_intervals(k)
    kmers = inside_counts(per_rec, seqs, k, iv)
    assert [int(x) for x in kmers[:6]] == [8191, 8192, 8193, 31, 32, 33] and int(kmers[6]) == 0, k      # the intervals are what they are for
    g = to_device(ctx, names, seqs)
    try:
        for rate in (1, 16):
            members = set_of_copy("copy", copy, k, rate)
            hs = HashSet(ctx, members)
            try:
                got, counts = g.hset_sample_intervals(hs, iv, k, rate)
            finally:
                hs.free()
            exp, exp_counts = oracle_sample(per_rec, seqs, k, members, iv, rate)
            print(f"k {k} rate {rate}: set of {members.size} hashes; {got.size} records, oracle {exp.size}; per interval {[int(c) for c in counts]}")
            assert got.dtype == SAMPLE_DTYPE and counts.dtype == np.uint64 and counts.shape == (len(iv),)
            assert np.array_equal(counts, exp_counts), (k, rate)
            assert got.size == exp.size and np.array_equal(got, exp), (k, rate)              # order, h0, iv and off
            if rate == 1:
                assert 0 < got.size < int(kmers.sum()), k                                        # never a vacuous match
            else:
                assert got.size > 0, k
        # the empty set: nothing; the genome's own hashes at rate 1: every valid k-mer
        none = HashSet(ctx, np.zeros(0, dtype=np.uint64))
        own = HashSet(ctx, np.concatenate([h for _, h in per_rec]))
        try:
            got0, counts0 = g.hset_sample_intervals(none, iv, k, 1)
            assert got0.size == 0 and not counts0.any(), k
            every, counts1 = g.hset_sample_intervals(own, iv, k, 1)
            assert np.array_equal(counts1, kmers) and every.size == int(kmers.sum()) > 0, k
            exp, _ = oracle_sample(per_rec, seqs, k, np.concatenate([h for _, h in per_rec]), iv, 1)
            assert np.array_equal(every, exp), k
            empty = g.hset_sample_intervals(own, np.zeros((0, 3), np.uint64), k, 16)
            assert empty[0].size == 0 and empty[1].size == 0
        finally:
            none.free()
            own.free()
    finally:
        g.free()


@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    from ntsynt_amd.device import HashSet
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], L.SUBSTITUTIONS, 1, seed=79, structural=False)]
    per_rec = kmers_of("end", seqs, k)
    kmers = inside_counts(per_rec, seqs, k, iv)
    assert [int(x) for x in kmers[:12]] == list(END_CASE_KMERS) * 2, k
    g = to_device(ctx, names, seqs)
    try:
        for rate in (1, 16):
            members = set_of_copy("end_copy", copy, k, rate)
            hs = HashSet(ctx, members)
            try:
                got, counts = g.hset_sample_intervals(hs, iv, k, rate)
            finally:
                hs.free()
            exp, exp_counts = oracle_sample(per_rec, seqs, k, members, iv, rate)
            print(f"k {k} rate {rate}: {got.size} records, oracle {exp.size}; per interval {[int(c) for c in counts]}")
            assert np.array_equal(counts, exp_counts), (k, rate)
            assert got.size == exp.size and np.array_equal(got, exp), (k, rate)              # order, h0, iv and off
            assert 0 < got.size < int(kmers.sum()), (k, rate)                                # never a vacuous match
    finally:
        g.free()


# ---- 3. slicing -----------------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_launch_takes_give_the_same_records(ctx_x, monkeypatch):
    from ntsynt_amd.device import HashSet
    names, seqs, copy = L.sample_inputs()
    k, rate = 24, 4
    per_rec = kmers_of("seqs", seqs, k)
    members = set_of_copy("copy", copy, k, rate)
    g = to_device(ctx_x, names, seqs)
    hs = HashSet(ctx_x, members)
    try:
        iv = L.sample_intervals(k) + [(0, a, a + 700) for a in range(0, 38_000, 500)]       # many short intervals as well
        ctx_x.profile(2)
        try:
            before = [ctx_x.timing(t)[1] for t in TIMERS]
            plain = g.hset_sample_intervals(hs, iv, k, rate)
            one = [ctx_x.timing(t)[1] - b for t, b in zip(TIMERS, before)]
            monkeypatch.setenv("NTS_HSET_SAMPLE_SLICE", "7")
            cut = g.hset_sample_intervals(hs, iv, k, rate)
            many = [ctx_x.timing(t)[1] - b - o for t, b, o in zip(TIMERS, before, one)]
        finally:
            ctx_x.profile(False)
        print(f"launches (count, write): {one} uncut, {many} with 7 tiles per launch")
        assert one == [1, 1] and many[0] == many[1] and many[0] > 10
        assert np.array_equal(plain[0], cut[0]) and np.array_equal(plain[1], cut[1])
        exp, exp_counts = oracle_sample(per_rec, seqs, k, members, iv, rate)
        assert np.array_equal(cut[0], exp) and np.array_equal(cut[1], exp_counts) and exp.size > 0
    finally:
        hs.free()
        g.free()


def test_the_launch_knob_is_not_in_the_product_build(ctx, monkeypatch):
    from ntsynt_amd.device import HashSet
    names, seqs, copy = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    hs = HashSet(ctx, set_of_copy("copy", copy, 24, 4))
    try:
        monkeypatch.setenv("NTS_HSET_SAMPLE_SLICE", "7")
        ctx.profile(2)
        try:
            before = [ctx.timing(t)[1] for t in TIMERS]
            got, _ = g.hset_sample_intervals(hs, L.sample_intervals(24), 24, 4)
            assert got.size > 0 and [ctx.timing(t)[1] - b for t, b in zip(TIMERS, before)] == [1, 1]
        finally:
            ctx.profile(False)
    finally:
        hs.free()
        g.free()


# ---- 4. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    from ntsynt_amd.device import HashSet, NtsError
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    hs = HashSet(ctx, np.arange(100, dtype=np.uint64))
    try:
        with pytest.raises(NtsError, match="record index out of range"):
            g.hset_sample_intervals(hs, [(0, 0, 10), (len(seqs), 0, 10)], 24, 16)
        with pytest.raises(NtsError, match="bad arguments"):
            g.hset_sample_intervals(hs, [(0, 0, 100)], 24, 0)
        hs.free()
        assert hs.h is None
        with pytest.raises(NtsError, match="nts_hset_sample_intervals: bad arguments"):      # a freed set is a NULL handle
            g.hset_sample_intervals(hs, [(0, 0, 100)], 24, 16)
        with pytest.raises(NtsError, match="nts_hset_contains: bad arguments"):
            hs.contains(np.arange(4, dtype=np.uint64))
        hs.free()                                                                            # twice: nothing happens
        ctx.lib.nts_hset_free(ctx.h, None)
    finally:
        hs.free()
        g.free()

"""The counting table beside the exact hash set (csrc/nts_hcount.inc): nts_hcount_add / nts_hcount_read against collections.Counter on
the sizes and keys at which the set's table can go wrong, one key added 100 000 times; nts_hset_count_intervals against the oracle --
O.hash_all of the record, the threshold, membership, np.unique's multiplicities -- on tests/test_gpu_hset.py's inputs and intervals; a
record with a tandem array and a segment held three times, once reverse-complemented; partial lanes up to the genome's last base; the
launch cut forced on the experiments build; the errors and the 2^32 guard.  Every test runs under a time limit of its own."""
import ctypes
import faulthandler
from collections import Counter

import numpy as np
import pytest

from ntsynt_amd import synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.helpers import END_CASE_KMERS, genome_end_case, to_device
from tests.helpers import oracle_set_sample as oracle_sample
from tests.test_gpu_hset import inside_counts, kmers_of, set_of_copy

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
U64_MAX = (1 << 64) - 1
TIMER = "hcount_sweep"


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


def u64(values):
    return np.asarray(values, dtype=np.uint64)


# ---- 1. the table alone ---------------------------------------------------------------------------------------------------------------
def check_table(ctx, keys, added, queries, what):
    "the set of `keys`, `added` offered to its counter, the counts of `queries` against a Counter restricted to the members"
    from ntsynt_amd.device import HashCounts, HashSet
    keys, added, queries = u64(keys), u64(added), u64(queries)
    members = set(int(x) for x in keys)
    seen = Counter(int(x) for x in added if int(x) in members)
    exp = np.array([seen.get(int(q), 0) for q in queries], dtype=np.uint32)
    hs = HashSet(ctx, keys)
    hc = HashCounts(ctx, hs)
    try:
        assert not hc.read(queries).any(), what                                 # counts start at zero
        hc.add(added)
        got = hc.read(queries)
    finally:
        hc.free()
        hs.free()
    print(f"{what}: {len(members)} members, {added.size} values added ({sum(seen.values())} of members), {queries.size} read, largest count {int(exp.max()) if exp.size else 0}")
    assert got.dtype == np.uint32 and got.shape == exp.shape, what
    assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:10])
    return got


def test_sizes_around_a_power_of_two_each_key_added_one_to_three_times(ctx):
    rng = np.random.default_rng(421)
    for n in (0, 1, 1023, 1024, 1025):
        keys = rng.integers(0, U64_MAX, size=n, dtype=np.uint64, endpoint=True)
        assert np.unique(keys).size == n
        times = rng.integers(1, 3, size=n, endpoint=True)
        added = rng.permutation(np.repeat(keys, times))
        others = rng.integers(0, U64_MAX, size=max(n, 8), dtype=np.uint64, endpoint=True)
        got = check_table(ctx, keys, np.concatenate([added, others]), np.concatenate([keys, others, u64([0, U64_MAX])]), f"n = {n}")
        assert np.array_equal(got[:n], times) and not got[n:].any()             # (non-members among the added values: nothing, and they read 0)
        if n >= 1023:
            assert set(int(t) for t in times) == {1, 2, 3}


def test_zero_and_all_ones_present_and_absent(ctx):
    rng = np.random.default_rng(422)
    some = rng.integers(1, U64_MAX, size=300, dtype=np.uint64)                  # neither 0 nor 2^64 - 1
    ends = u64([0, U64_MAX, 1, U64_MAX - 1])
    added = np.concatenate([some, u64([0] * 5 + [U64_MAX] * 7 + [1, U64_MAX - 1])])
    for with_zero in (False, True):
        for with_max in (False, True):
            keys = np.concatenate([some, u64([0] * with_zero + [U64_MAX] * with_max)])
            got = check_table(ctx, keys, added, np.concatenate([ends, some]), f"0 {'in' if with_zero else 'out'}, 2^64 - 1 {'in' if with_max else 'out'}")
            assert [int(x) for x in got[:4]] == [5 * with_zero, 7 * with_max, 0, 0] and (got[4:] == 1).all()
    assert [int(x) for x in check_table(ctx, [U64_MAX], added, ends, "2^64 - 1 alone")] == [0, 7, 0, 0]
    assert [int(x) for x in check_table(ctx, [0], added, ends, "0 alone")] == [5, 0, 0, 0]
    assert [int(x) for x in check_table(ctx, [], added, ends, "the empty set")] == [0, 0, 0, 0]


def test_keys_that_differ_in_few_bits(ctx):
    rng = np.random.default_rng(423)
    i = np.arange(4096, dtype=np.uint64)
    base = np.uint64(0x0005A5A5A5A5A000)                                        # low 12 and top 12 bits clear
    low = base | i
    top = base | (i << np.uint64(52))
    assert np.unique(low >> np.uint64(12)).size == 1 and np.unique(top & np.uint64((1 << 52) - 1)).size == 1
    for what, keys in (("low 12 bits", low), ("top 12 bits", top)):
        half = keys[::2]                                                       # every other one is a member; the rest are near misses
        times = rng.integers(1, 3, size=keys.size, endpoint=True)
        got = check_table(ctx, half, rng.permutation(np.repeat(keys, times)), keys, what)
        assert np.array_equal(got[::2], times[::2]) and not got[1::2].any()


def test_one_key_added_100000_times_among_1000_others(ctx):
    "every add of the hot key goes to one address: exactly 100 000"
    rng = np.random.default_rng(424)
    keys = rng.integers(0, U64_MAX, size=1001, dtype=np.uint64, endpoint=True)
    assert np.unique(keys).size == 1001
    added = rng.permutation(np.concatenate([np.full(100_000, keys[0], dtype=np.uint64), keys[1:]]))
    got = check_table(ctx, keys, added, keys, "one hot key")
    assert int(got[0]) == 100_000 and (got[1:] == 1).all()


def test_clear_zeroes_everything_and_two_adds_accumulate(ctx):
    from ntsynt_amd.device import HashCounts, HashSet
    rng = np.random.default_rng(425)
    keys = rng.integers(0, U64_MAX, size=5000, dtype=np.uint64, endpoint=True)
    keys[0], keys[1] = 0, U64_MAX
    hs = HashSet(ctx, keys)
    hc = HashCounts(ctx, hs)
    try:
        hc.add(keys)
        hc.add(keys[:2000])
        hc.add(np.zeros(0, dtype=np.uint64))
        got = hc.read(keys)
        assert (got[:2000] == 2).all() and (got[2000:] == 1).all()
        hc.clear()
        assert not hc.read(keys).any()
        hc.add(keys[1000:3000])
        got = hc.read(keys)
        assert not got[:1000].any() and (got[1000:3000] == 1).all() and not got[3000:].any()
        assert hc.read(np.zeros(0, dtype=np.uint64)).size == 0
    finally:
        hc.free()
        hs.free()


# ---- 2. the sweep ---------------------------------------------------------------------------------------------------------------------
def oracle_counts(per_rec, seqs, k, members, intervals, rate):
    """(keys, counts, hits per interval) by the definitions: the k-mers wholly inside each interval, under the threshold, restricted to
    the members, np.unique's multiplicities summed over the intervals (oracle_set_sample's records are exactly those k-mers, once per
    interval that holds them)"""
    recs, hits = oracle_sample(per_rec, seqs, k, members, intervals, rate)
    keys, counts = np.unique(recs["h0"], return_counts=True)
    return keys, counts.astype(np.uint32), hits


def expected_for(members, keys, counts):
    "the counts of `members` (distinct, sorted), 0 for those the sweep did not meet"
    exp = np.zeros(members.size, dtype=np.uint32)
    exp[np.searchsorted(members, keys)] = counts
    return exp


def sweep_and_compare(g, hs, hc, members, per_rec, seqs, k, iv, rate, what):
    "one cleared sweep against the oracle: hits per interval, the count of every member, zero for near misses; returns (hits, counts)"
    members = np.unique(members)
    hc.clear()
    hits = g.hset_count_intervals(hs, hc, iv, k, rate)
    got = hc.read(members)
    keys, counts, exp_hits = oracle_counts(per_rec, seqs, k, members, iv, rate)
    exp = expected_for(members, keys, counts)
    print(f"{what}: set of {members.size}; hits {int(hits.sum())} (oracle {int(exp_hits.sum())}); members met {int((got > 0).sum())}, largest count {int(got.max()) if got.size else 0}")
    assert hits.dtype == np.uint64 and hits.shape == (len(iv),), what
    assert np.array_equal(hits, exp_hits), what
    assert np.array_equal(got, exp), (what, np.flatnonzero(got != exp)[:10])
    assert int(got.sum()) == int(hits.sum()), what                              # every hit is one add
    assert not hc.read(members ^ np.uint64(1 << 30))[~np.isin(members ^ np.uint64(1 << 30), members)].any(), what
    return hits, got


@pytest.mark.parametrize("k", KS)
def test_sweep_equals_the_oracle(ctx, k):
    from ntsynt_amd.device import HashCounts, HashSet
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
            hc = HashCounts(ctx, hs)
            try:
                hits, got = sweep_and_compare(g, hs, hc, members, per_rec, seqs, k, iv, rate, f"k {k} rate {rate}")
                if rate == 1:
                    assert 0 < int(hits.sum()) < int(kmers.sum()), k                             # never a vacuous match
                else:
                    assert int(hits.sum()) > 0, k
                assert int(got.max()) >= 2                                                       # overlapping intervals count a k-mer once each
                # a second sweep without a clear accumulates
                again = g.hset_count_intervals(hs, hc, iv, k, rate)
                assert np.array_equal(again, hits) and np.array_equal(hc.read(np.unique(members)), 2 * got), (k, rate)
            finally:
                hc.free()
                hs.free()
        # the empty set: nothing; the genome's own hashes at rate 1: every count is the oracle's multiplicity; no interval
        own_h = np.concatenate([h for _, h in per_rec])
        none = HashSet(ctx, np.zeros(0, dtype=np.uint64))
        none_c = HashCounts(ctx, none)
        own = HashSet(ctx, own_h)
        own_c = HashCounts(ctx, own)
        try:
            assert not g.hset_count_intervals(none, none_c, iv, k, 1).any(), k
            assert not none_c.read(own_h[:100]).any(), k
            hits, _ = sweep_and_compare(g, own, own_c, own_h, per_rec, seqs, k, iv, 1, f"k {k}: the genome's own set")
            assert np.array_equal(hits, kmers) and int(kmers.sum()) > 0, k
            whole = [(r, 0, len(s)) for r, s in enumerate(seqs)]
            own_c.clear()
            hits = g.hset_count_intervals(own, own_c, whole, k, 1)
            keys, mult = np.unique(own_h, return_counts=True)
            assert np.array_equal(own_c.read(keys), mult.astype(np.uint32)) and int(hits.sum()) == own_h.size, k
            own_c.clear()
            empty = g.hset_count_intervals(own, own_c, np.zeros((0, 3), np.uint64), k, 16)
            assert empty.size == 0 and not own_c.read(keys).any(), k
        finally:
            none_c.free()
            own_c.free()
            none.free()
            own.free()
    finally:
        g.free()


# ---- 3. multiplicities above one -------------------------------------------------------------------------------------------------------
def repeat_record():
    "random bases with a 37-base unit repeated 60 times and a 2 000-base segment present three times, the third reverse-complemented"
    rng = np.random.default_rng(426)
    unit, segment = synth.random_dna(37, rng), synth.random_dna(2_000, rng)
    parts = [synth.random_dna(9_001, rng), np.tile(unit, 60), synth.random_dna(5_003, rng), segment, synth.random_dna(7_019, rng), segment,
             synth.random_dna(4_507, rng), synth.revcomp(segment), synth.random_dna(3_011, rng)]
    return np.concatenate(parts).tobytes()


def test_a_tandem_array_and_a_segment_held_three_times(ctx):
    from ntsynt_amd.device import HashCounts, HashSet
    k = 24
    seq = repeat_record()
    pos, h0 = O.hash_all(seq, k)
    assert pos.size == len(seq) - k + 1
    keys, mult = np.unique(h0, return_counts=True)
    g = to_device(ctx, ["rep"], [seq])
    hs = HashSet(ctx, h0)
    hc = HashCounts(ctx, hs)
    try:
        hits = g.hset_count_intervals(hs, hc, [(0, 0, len(seq))], k, 1)
        got = hc.read(keys)
        print(f"{h0.size} k-mers, {keys.size} distinct; largest count {int(got.max())}, {int((got == 3).sum())} members with count 3")
        assert int(hits[0]) == h0.size
        assert np.array_equal(got, mult.astype(np.uint32))
        assert int(got.max()) >= 50                                             # the tandem array: 37 k-mers, some 59 times each
        assert int((got == 3).sum()) >= 1900                                    # the segment: the canonical hash counts the third copy too
    finally:
        hc.free()
        hs.free()
        g.free()


# ---- 4. partial lanes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    from ntsynt_amd.device import HashCounts, HashSet
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
            hc = HashCounts(ctx, hs)
            try:
                hits, _ = sweep_and_compare(g, hs, hc, members, per_rec, seqs, k, iv, rate, f"k {k} rate {rate}")
                assert 0 < int(hits.sum()) < int(kmers.sum()), (k, rate)                         # never a vacuous match
            finally:
                hc.free()
                hs.free()
    finally:
        g.free()


# ---- 5. slicing -----------------------------------------------------------------------------------------------------------------------
def test_more_tiles_than_one_launch_takes_give_the_same_counts(ctx_x, monkeypatch):
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    k, rate = 24, 4
    per_rec = kmers_of("seqs", seqs, k)
    members = np.unique(set_of_copy("copy", copy, k, rate))
    g = to_device(ctx_x, names, seqs)
    hs = HashSet(ctx_x, members)
    hc = HashCounts(ctx_x, hs)
    try:
        iv = L.sample_intervals(k) + [(0, a, a + 700) for a in range(0, 38_000, 500)]       # many short intervals as well
        ctx_x.profile(2)
        try:
            before = ctx_x.timing(TIMER)[1]
            plain_hits = g.hset_count_intervals(hs, hc, iv, k, rate)
            plain = hc.read(members)
            one = ctx_x.timing(TIMER)[1] - before
            monkeypatch.setenv("NTS_HSET_COUNT_SLICE", "7")
            hc.clear()
            cut_hits = g.hset_count_intervals(hs, hc, iv, k, rate)
            cut = hc.read(members)
            many = ctx_x.timing(TIMER)[1] - before - one
        finally:
            ctx_x.profile(False)
        print(f"launches: {one} uncut, {many} with 7 tiles per launch")
        assert one == 1 and many > 10
        assert np.array_equal(plain, cut) and np.array_equal(plain_hits, cut_hits)
        keys, counts, exp_hits = oracle_counts(per_rec, seqs, k, members, iv, rate)
        assert np.array_equal(cut, expected_for(members, keys, counts)) and np.array_equal(cut_hits, exp_hits) and int(exp_hits.sum()) > 0
    finally:
        hc.free()
        hs.free()
        g.free()


def test_the_launch_knob_is_not_in_the_product_build(ctx, monkeypatch):
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    hs = HashSet(ctx, set_of_copy("copy", copy, 24, 4))
    hc = HashCounts(ctx, hs)
    try:
        monkeypatch.setenv("NTS_HSET_COUNT_SLICE", "7")
        ctx.profile(2)
        try:
            before = ctx.timing(TIMER)[1]
            hits = g.hset_count_intervals(hs, hc, L.sample_intervals(24), 24, 4)
            assert int(hits.sum()) > 0 and ctx.timing(TIMER)[1] - before == 1
        finally:
            ctx.profile(False)
    finally:
        hc.free()
        hs.free()
        g.free()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx):
    from ntsynt_amd.device import HashCounts, HashSet, NtsError
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    keys = np.arange(100, dtype=np.uint64)
    hs, other = HashSet(ctx, keys), HashSet(ctx, keys)
    hc = HashCounts(ctx, hs)
    try:
        with pytest.raises(NtsError, match="record index out of range"):
            g.hset_count_intervals(hs, hc, [(0, 0, 100), (len(seqs), 0, 100)], 24, 16)
        with pytest.raises(NtsError, match="nts_hset_count_intervals: bad arguments"):
            g.hset_count_intervals(hs, hc, [(0, 0, 100)], 24, 0)
        # a counter used with a set other than its own, equal though that set is
        hc.hset = other
        for call in (lambda: hc.add(keys), lambda: hc.read(keys), lambda: g.hset_count_intervals(other, hc, [(0, 0, 100)], 24, 16)):
            with pytest.raises(NtsError, match="the counter belongs to another set"):
                call()
        hc.hset = hs
        hc.add(keys)
        assert (hc.read(keys) == 1).all()                                      # none of the refused calls counted anything
        # a freed counter, a freed set: NULL handles
        hc.free()
        assert hc.h is None
        for call, name in ((lambda: hc.add(keys), "nts_hcount_add"), (lambda: hc.read(keys), "nts_hcount_read"), (hc.clear, "nts_hcount_clear"),
                           (lambda: g.hset_count_intervals(hs, hc, [(0, 0, 100)], 24, 16), "nts_hset_count_intervals")):
            with pytest.raises(NtsError, match=name + ": bad arguments"):
                call()
        hc.free()                                                               # twice: nothing happens
        ctx.lib.nts_hcount_free(ctx.h, None)
        hc = HashCounts(ctx, hs)
        other.free()
        with pytest.raises(NtsError, match="nts_hcount_create: bad arguments"):
            HashCounts(ctx, other)
        hc.hset = other
        with pytest.raises(NtsError, match="nts_hcount_add: bad arguments"):
            hc.add(keys)
        with pytest.raises(NtsError, match="nts_hset_count_intervals: bad arguments"):
            g.hset_count_intervals(other, hc, [(0, 0, 100)], 24, 16)
        hc.hset = hs
    finally:
        hc.free()
        hs.free()
        other.free()
        g.free()


def test_a_counter_is_not_offered_2_to_the_32(ctx):
    """the guard is the counter's host total: a call that would bring it to 2^32 is refused before anything is launched and before the
    values are looked at -- so the refused calls below pass a count far beyond the array they point at"""
    from ntsynt_amd.device import HashCounts, HashSet, NtsError
    names, seqs, _ = L.sample_inputs()
    keys = np.arange(1000, dtype=np.uint64)
    hs = HashSet(ctx, keys)
    hc = HashCounts(ctx, hs)
    g = to_device(ctx, names, seqs)

    def offer(n):
        "nts_hcount_add with a claimed count of n"
        return ctx.lib.nts_hcount_add(ctx.h, hs.h, hc.h, keys.ctypes.data, ctypes.c_uint64(n))
    try:
        for n in (1 << 32, (1 << 32) + 5, U64_MAX):
            assert offer(n) != 0
            with pytest.raises(NtsError, match="2\\^32 values and k-mers or more since the last clear"):
                ctx.check(offer(n), "nts_hcount_add")
        hc.add(keys)                                                            # total 1000
        assert offer((1 << 32) - 1000) != 0                                     # would make it 2^32 exactly
        whole = [(r, 0, len(s)) for r, s in enumerate(seqs)]
        hits = g.hset_count_intervals(hs, hc, whole, 24, 1)                     # the sweep's k-mers go into the same total
        n_kmers = sum(int(p.size) for p, _ in kmers_of("seqs", seqs, 24))
        assert n_kmers > 70_000 and int(hits.sum()) <= n_kmers
        assert offer((1 << 32) - 1000 - n_kmers) != 0                           # exactly 2^32 again: the sweep offered every one of its k-mers
        assert (hc.read(keys) >= 1).all() and int(hc.read(keys).sum()) == 1000 + int(hits.sum())      # nothing of the refused calls was counted
        hc.clear()                                                              # the total goes with the counts
        hc.add(keys)
        assert (hc.read(keys) == 1).all()
    finally:
        hc.free()
        hs.free()
        g.free()

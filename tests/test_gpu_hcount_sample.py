"""The capped sampling sweep (csrc/nts_hcount.inc, nts_hset_sample_intervals_capped): nts_hset_sample_intervals that keeps a k-mer only
when its count in the set's counter lies in 1..cap.  Against the oracle -- oracle_set_sample's records, kept where np.unique's
multiplicity over the counted intervals lies within 1..cap -- on tests/test_gpu_hcount.py's inputs and intervals; the largest cap
against the uncapped sweep; the repeat record's tandem array and triple segment on either side of their caps; a cleared counter and a
counter swept twice; partial lanes and the tile sizes; the launch cut on the experiments build; the errors; the counter untouched.
Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from ntsynt_amd import synth
from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.helpers import END_CASE_KMERS, genome_end_case, to_device
from tests.helpers import oracle_set_sample as oracle_sample
from tests.test_gpu_hcount import repeat_record
from tests.test_gpu_hset import inside_counts, kmers_of, set_of_copy

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
CAPS = [1, 2, 3, (1 << 32) - 1]
TIMERS = ("hcount_sample_count", "hcount_sample_write")


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


def capped(recs, cap, sweeps=1):
    """(records, per-interval counts) of the oracle's records `recs` (those of the counted intervals) kept where the multiplicity of
    their hash among them, times the number of count sweeps, lies within 1..cap"""
    keys, inverse, mult = np.unique(recs["h0"], return_inverse=True, return_counts=True)
    keep = mult[inverse] * sweeps <= cap
    return recs[keep], keep


def per_interval(recs, n_iv):
    return np.bincount(recs["iv"].astype(np.int64), minlength=n_iv).astype(np.uint64)


@pytest.mark.parametrize("k", KS)
def test_capped_sweep_equals_the_oracle(ctx, k):
    from ntsynt_amd.device import SAMPLE_DTYPE, HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    per_rec = kmers_of("seqs", seqs, k)
    iv = L.sample_intervals(k)
    kmers = inside_counts(per_rec, seqs, k, iv)
    assert [int(x) for x in kmers[:6]] == [8191, 8192, 8193, 31, 32, 33] and int(kmers[6]) == 0, k      # the intervals are what they are for
    g = to_device(ctx, names, seqs)
    try:
        for rate in (1, 16):
            members = set_of_copy("copy", copy, k, rate)
            exp_all, exp_all_counts = oracle_sample(per_rec, seqs, k, members, iv, rate)
            mult = np.unique(exp_all["h0"], return_counts=True)[1]
            assert int(mult.max()) >= 2, (k, rate)                                  # overlapping intervals: some k-mer is counted twice
            hs = HashSet(ctx, members)
            hc = HashCounts(ctx, hs)
            try:
                g.hset_count_intervals(hs, hc, iv, k, rate)
                sizes = []
                for cap in CAPS:
                    got, counts = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
                    exp, _ = capped(exp_all, cap)
                    print(f"k {k} rate {rate} cap {cap}: {got.size} records, oracle {exp.size} of {exp_all.size} uncapped")
                    assert got.dtype == SAMPLE_DTYPE and counts.dtype == np.uint64 and counts.shape == (len(iv),)
                    assert np.array_equal(counts, per_interval(exp, len(iv))), (k, rate, cap)
                    assert got.size == exp.size and np.array_equal(got, exp), (k, rate, cap)     # order, h0, iv and off
                    sizes.append(got.size)
                assert 0 < sizes[0] < sizes[1] <= sizes[2] <= sizes[3] == exp_all.size, (k, rate, sizes)       # the cap cuts, never vacuously
                # the largest cap after a count sweep of the same intervals: the uncapped sweep, record for record
                plain, plain_counts = g.hset_sample_intervals(hs, iv, k, rate)
                assert np.array_equal(got, plain) and np.array_equal(counts, plain_counts) and np.array_equal(plain_counts, exp_all_counts), (k, rate)
                empty = g.hset_sample_intervals_capped(hs, hc, 3, np.zeros((0, 3), np.uint64), k, rate)
                assert empty[0].size == 0 and empty[1].size == 0
            finally:
                hc.free()
                hs.free()
    finally:
        g.free()


def test_the_tandem_array_and_the_triple_segment_on_either_side_of_their_caps(ctx):
    "a 37-base unit x 60 (its k-mers up to 60 times), a 2 000-base segment held three times, once reverse-complemented (1 977 k-mers x 3)"
    from ntsynt_amd.device import HashCounts, HashSet
    k = 24
    seq = repeat_record()
    pos, h0 = O.hash_all(seq, k)
    keys, inverse, mult = np.unique(h0, return_inverse=True, return_counts=True)
    assert int(mult.max()) == 60 and int((mult == 3).sum()) >= 1977 and not ((mult > 3) & (mult < 59)).any()
    whole = [(0, 0, len(seq))]
    g = to_device(ctx, ["rep"], [seq])
    hs = HashSet(ctx, h0)
    hc = HashCounts(ctx, hs)
    try:
        g.hset_count_intervals(hs, hc, whole, k, 1)
        sizes = {}
        for cap in (1, 2, 3, 58, 59, 60):
            got, counts = g.hset_sample_intervals_capped(hs, hc, cap, whole, k, 1)
            keep = mult[inverse] <= cap
            assert got.size == int(keep.sum()) == int(counts[0]), cap
            assert np.array_equal(got["h0"], h0[keep]) and np.array_equal(got["off"], pos[keep].astype(np.uint32)) and not got["iv"].any(), cap
            sizes[cap] = got.size
        print("records per cap:", sizes)
        assert sizes[3] - sizes[2] == 3 * int((mult == 3).sum()) >= 3 * 1977                   # cap 2 leaves the triple members out, cap 3 takes them in
        assert sizes[60] - sizes[59] == 60 * int((mult == 60).sum()) > 0                        # cap 59 leaves the tandem's 60-fold members out, cap 60 takes them in
        assert sizes[60] == h0.size and sizes[1] == int((mult == 1).sum())
    finally:
        hc.free()
        hs.free()
        g.free()


def test_a_cleared_counter_gives_nothing_and_a_second_sweep_halves_what_a_cap_admits(ctx):
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    k, rate = 24, 1
    per_rec = kmers_of("seqs", seqs, k)
    iv = L.sample_intervals(k)
    members = set_of_copy("copy", copy, k, rate)
    exp_all, _ = oracle_sample(per_rec, seqs, k, members, iv, rate)
    g = to_device(ctx, names, seqs)
    hs = HashSet(ctx, members)
    hc = HashCounts(ctx, hs)
    try:
        for cap in (1, (1 << 32) - 1):                                             # counts start at zero, and are zero again after clear()
            got, counts = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
            assert got.size == 0 and not counts.any(), cap
        g.hset_count_intervals(hs, hc, iv, k, rate)
        g.hset_count_intervals(hs, hc, iv, k, rate)                                # every count doubled
        for cap in (1, 2, 3, 4):
            got, _ = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
            exp, _ = capped(exp_all, cap, sweeps=2)
            assert np.array_equal(got, exp), cap
            assert np.array_equal(got, capped(exp_all, cap // 2)[0] if cap >= 2 else exp_all[:0]), cap
        assert exp.size > 0
        hc.clear()
        got, counts = g.hset_sample_intervals_capped(hs, hc, 4, iv, k, rate)
        assert got.size == 0 and not counts.any()
    finally:
        hc.free()
        hs.free()
        g.free()


@pytest.mark.parametrize("k", [150, 24])
def test_partial_lanes_up_to_the_last_base_of_the_genome(ctx, k):
    "k = 150: every lane reads its own bases and a partial one rolls on past the tile; k = 24: the same intervals through the staging area"
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, iv = genome_end_case(k)
    copy = [c.tobytes() for c in synth.derive_genome([np.frombuffer(s, dtype=np.uint8) for s in seqs], L.SUBSTITUTIONS, 1, seed=79, structural=False)]
    per_rec = kmers_of("end", seqs, k)
    kmers = inside_counts(per_rec, seqs, k, iv)
    assert [int(x) for x in kmers[:12]] == list(END_CASE_KMERS) * 2, k         # 1 / 31 / 33 / 8191 / 8192 / 8193 k-mers, twice
    g = to_device(ctx, names, seqs)
    try:
        for rate in (1, 16):
            members = set_of_copy("end_copy", copy, k, rate)
            exp_all, _ = oracle_sample(per_rec, seqs, k, members, iv, rate)
            hs = HashSet(ctx, members)
            hc = HashCounts(ctx, hs)
            try:
                g.hset_count_intervals(hs, hc, iv, k, rate)
                for cap in (1, 2, 6):                                              # (the six intervals that end on the last base are nested)
                    got, counts = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
                    exp, _ = capped(exp_all, cap)
                    print(f"k {k} rate {rate} cap {cap}: {got.size} records, oracle {exp.size} of {exp_all.size}")
                    assert np.array_equal(counts, per_interval(exp, len(iv))), (k, rate, cap)
                    assert np.array_equal(got, exp), (k, rate, cap)
                    assert 0 < got.size <= exp_all.size, (k, rate, cap)
                assert got.size > capped(exp_all, 1)[0].size, (k, rate)            # the caps differ on this input
            finally:
                hc.free()
                hs.free()
    finally:
        g.free()


def test_more_tiles_than_one_launch_takes_give_the_same_records(ctx_x, monkeypatch):
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    k, rate, cap = 24, 4, 2
    per_rec = kmers_of("seqs", seqs, k)
    members = set_of_copy("copy", copy, k, rate)
    g = to_device(ctx_x, names, seqs)
    hs = HashSet(ctx_x, members)
    hc = HashCounts(ctx_x, hs)
    try:
        iv = L.sample_intervals(k) + [(0, a, a + 700) for a in range(0, 38_000, 500)]       # many short intervals as well
        g.hset_count_intervals(hs, hc, iv, k, rate)
        ctx_x.profile(2)
        try:
            before = [ctx_x.timing(t)[1] for t in TIMERS]
            plain = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
            one = [ctx_x.timing(t)[1] - b for t, b in zip(TIMERS, before)]
            monkeypatch.setenv("NTS_HSET_SAMPLE_SLICE", "7")
            cut = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
            many = [ctx_x.timing(t)[1] - b - o for t, b, o in zip(TIMERS, before, one)]
        finally:
            ctx_x.profile(False)
        print(f"launches (count, write): {one} uncut, {many} with 7 tiles per launch")
        assert one == [1, 1] and many[0] == many[1] and many[0] > 10
        assert np.array_equal(plain[0], cut[0]) and np.array_equal(plain[1], cut[1])
        exp_all, _ = oracle_sample(per_rec, seqs, k, members, iv, rate)
        exp, _ = capped(exp_all, cap)
        assert np.array_equal(cut[0], exp) and np.array_equal(cut[1], per_interval(exp, len(iv))) and 0 < exp.size < exp_all.size
    finally:
        hc.free()
        hs.free()
        g.free()


def test_errors(ctx):
    from ntsynt_amd.device import HashCounts, HashSet, NtsError
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    keys = np.arange(100, dtype=np.uint64)
    hs, other = HashSet(ctx, keys), HashSet(ctx, keys)
    hc = HashCounts(ctx, hs)
    try:
        with pytest.raises(NtsError, match="the counter belongs to another set"):             # equal though that set is
            g.hset_sample_intervals_capped(other, hc, 16, [(0, 0, 100)], 24, 16)
        with pytest.raises(NtsError, match="nts_hset_sample_intervals_capped: bad arguments"):
            g.hset_sample_intervals_capped(hs, hc, 0, [(0, 0, 100)], 24, 16)
        with pytest.raises(NtsError, match="nts_hset_sample_intervals_capped: bad arguments"):
            g.hset_sample_intervals_capped(hs, hc, 16, [(0, 0, 100)], 24, 0)
        with pytest.raises(NtsError, match="record index out of range"):
            g.hset_sample_intervals_capped(hs, hc, 16, [(0, 0, 100), (len(seqs), 0, 100)], 24, 16)
        got, counts = g.hset_sample_intervals_capped(hs, hc, 16, [(0, 0, 100)], 24, 16)      # and the accepted call beside them
        assert got.size == 0 and counts.shape == (1,)
        hc.free()
        with pytest.raises(NtsError, match="nts_hset_sample_intervals_capped: bad arguments"):  # a freed counter is a NULL handle
            g.hset_sample_intervals_capped(hs, hc, 16, [(0, 0, 100)], 24, 16)
    finally:
        hc.free()
        hs.free()
        other.free()
        g.free()


def test_the_counter_and_what_it_was_offered_are_untouched(ctx):
    "the counts read the same before and after; the running total too: the call that would bring it to 2^32 is refused before and after alike"
    import ctypes
    from ntsynt_amd.device import HashCounts, HashSet
    names, seqs, copy = L.sample_inputs()
    k, rate = 24, 1
    members = np.unique(set_of_copy("copy", copy, k, rate))
    iv = L.sample_intervals(k)
    n_kmers = int(inside_counts(kmers_of("seqs", seqs, k), seqs, k, iv).sum())
    g = to_device(ctx, names, seqs)
    hs = HashSet(ctx, members)
    hc = HashCounts(ctx, hs)

    def offer(n):
        "nts_hcount_add with a claimed count of n: refused, before the values are looked at, when the total would reach 2^32"
        return ctx.lib.nts_hcount_add(ctx.h, hs.h, hc.h, members.ctypes.data, ctypes.c_uint64(n))
    try:
        g.hset_count_intervals(hs, hc, iv, k, rate)                                # offered: every k-mer of the intervals
        before = hc.read(members)
        assert offer((1 << 32) - n_kmers) != 0                                     # exactly 2^32: refused
        for cap in (1, 3, (1 << 32) - 1):
            got, _ = g.hset_sample_intervals_capped(hs, hc, cap, iv, k, rate)
            assert got.size > 0
        assert np.array_equal(hc.read(members), before) and int(before.sum()) > 0
        assert offer((1 << 32) - n_kmers) != 0                                     # still exactly 2^32 ...
        hc.add(members[:1])                                                        # ... and one value is still accepted: the total did not move
        after = hc.read(members)
        assert int(after[0]) == int(before[0]) + 1 and np.array_equal(after[1:], before[1:])
    finally:
        hc.free()
        hs.free()
        g.free()

"""The sampler that probes nothing (csrc/nts_iv_sample.inc, nts_sample_intervals) against its definition -- O.hash_all of the record,
wholly inside the clipped interval, h0 <= (2^64 - 1) // rate -- array for array on the end-case family of tests/helpers.py (partial lanes,
8191 / 8192 / 8193 k-mers, intervals that end on the genome's last base, one across the N run); against nts_bf_sample_intervals with a
filter of all ones, record for record; the launch cut forced on the experiments build; the empty answers; the errors; the same bytes
twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from oracle import nts_oracle as O
from tests import test_gpu_gap_links as L
from tests.helpers import END_CASE_KMERS, genome_end_case, oracle_set_sample, to_device

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
KS = [16, 24, 64, 150]
TIMERS = ("iv_sample_count", "iv_sample_write")
U64_MAX = (1 << 64) - 1


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


_hashes = {}


def kmers_of(tag, seqs, k):
    "per record (positions, hashes) by the oracle, once per input and k"
    if (tag, k) not in _hashes:
        _hashes[(tag, k)] = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in seqs)]
    return _hashes[(tag, k)]


def expected(per_rec, seqs, k, iv, rate):
    "the definition: oracle_set_sample with every hash of the records a member"
    return oracle_set_sample(per_rec, seqs, k, np.concatenate([h for _, h in per_rec]), iv, rate)


@pytest.mark.parametrize("k", KS)
def test_end_cases_equal_the_definition(ctx, k):
    from ntsynt_amd.device import SAMPLE_DTYPE
    names, seqs, iv = genome_end_case(k)
    per_rec = kmers_of("end", seqs, k)
    g = to_device(ctx, names, seqs)
    try:
        for rate in (1, 16):
            got, counts = g.sample_intervals(iv, k, rate)
            exp, exp_counts = expected(per_rec, seqs, k, iv, rate)
            print(f"k {k} rate {rate}: {got.size} records, definition {exp.size}; per interval {[int(c) for c in counts]}")
            assert got.dtype == SAMPLE_DTYPE and counts.dtype == np.uint64 and counts.shape == (len(iv),)
            assert np.array_equal(counts, exp_counts), (k, rate)                             # n_sampled
            assert got.size == exp.size and np.array_equal(got, exp), (k, rate)              # order, h0, iv and off
            if rate == 1:
                assert [int(c) for c in counts[:12]] == list(END_CASE_KMERS) * 2, k          # every valid k-mer, none beyond the lane's last
            else:
                assert 0 < got.size < exp_counts.size * 8193 and int(got["h0"].max()) <= U64_MAX // 16, k
    finally:
        g.free()


@pytest.mark.parametrize("k", [24, 150])
def test_a_filter_of_all_ones_gives_the_same_records(ctx, k):
    from ntsynt_amd.device import BloomFilter
    names, seqs, _ = L.sample_inputs()
    iv = L.sample_intervals(k)
    g = to_device(ctx, names, seqs)
    bf = BloomFilter(ctx, 4096, k, ones=True)
    try:
        for rate in (1, 16):
            plain, plain_counts = g.sample_intervals(iv, k, rate)
            held, held_counts = g.bf_sample_intervals(bf, iv, k, rate)
            print(f"k {k} rate {rate}: {plain.size} records without a filter, {held.size} with one of all ones")
            assert plain.size == held.size > 0 and np.array_equal(plain, held), (k, rate)
            assert np.array_equal(plain_counts, held_counts), (k, rate)
        exp, exp_counts = expected(kmers_of("seqs", seqs, k), seqs, k, iv, 16)
        assert np.array_equal(plain, exp) and np.array_equal(plain_counts, exp_counts), k
    finally:
        bf.free()
        g.free()


def test_more_tiles_than_one_launch_takes_give_the_same_records(ctx_x, monkeypatch):
    names, seqs, _ = L.sample_inputs()
    k, rate = 24, 4
    g = to_device(ctx_x, names, seqs)
    try:
        iv = L.sample_intervals(k) + [(0, a, a + 700) for a in range(0, 38_000, 500)]       # many short intervals as well
        ctx_x.profile(2)
        try:
            before = [ctx_x.timing(t)[1] for t in TIMERS]
            plain = g.sample_intervals(iv, k, rate)
            one = [ctx_x.timing(t)[1] - b for t, b in zip(TIMERS, before)]
            monkeypatch.setenv("NTS_IV_SAMPLE_SLICE", "7")
            cut = g.sample_intervals(iv, k, rate)
            many = [ctx_x.timing(t)[1] - b - o for t, b, o in zip(TIMERS, before, one)]
        finally:
            ctx_x.profile(False)
        print(f"launches (count, write): {one} uncut, {many} with 7 tiles per launch")
        assert one == [1, 1] and many[0] == many[1] and many[0] > 10
        assert np.array_equal(plain[0], cut[0]) and np.array_equal(plain[1], cut[1])
        exp, exp_counts = expected(kmers_of("seqs", seqs, k), seqs, k, iv, rate)
        assert np.array_equal(cut[0], exp) and np.array_equal(cut[1], exp_counts) and exp.size > 0
    finally:
        g.free()


def test_the_launch_knob_is_not_in_the_product_build(ctx, monkeypatch):
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    try:
        monkeypatch.setenv("NTS_IV_SAMPLE_SLICE", "7")
        ctx.profile(2)
        try:
            before = [ctx.timing(t)[1] for t in TIMERS]
            got, _ = g.sample_intervals(L.sample_intervals(24), 24, 4)
            assert got.size > 0 and [ctx.timing(t)[1] - b for t, b in zip(TIMERS, before)] == [1, 1]
        finally:
            ctx.profile(False)
    finally:
        g.free()


def test_nothing_to_sample(ctx):
    import ctypes
    from ntsynt_amd import _lib
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    try:
        for what, iv in (("shorter than k", [(0, 100, 123), (2, 5, 6), (1, 900, 900)]), ("beyond the record's end", [(2, 13_000, 14_000)]),
                         ("no interval", np.zeros((0, 3), np.uint64))):
            arr = g._interval_array(iv)
            counts = np.full(arr.size, 77, dtype=np.uint64)
            p, m = _lib.c_vp(12345), _lib.u64(99)
            rc = ctx.lib.nts_sample_intervals(ctx.h, g.h, 24, 1, ctypes.cast(arr.ctypes.data, ctypes.POINTER(_lib.Interval)), arr.size, counts.ctypes.data,
                                              ctypes.byref(p), ctypes.byref(m))
            assert rc == 0 and p.value is None and m.value == 0 and not counts.any(), what    # (NULL, 0) and zero counts
            got, c = g.sample_intervals(iv, 24, 1)
            assert got.size == 0 and c.shape == (arr.size,) and not c.any(), what
    finally:
        g.free()


def test_errors(ctx):
    from ntsynt_amd.device import NtsError
    names, seqs, _ = L.sample_inputs()
    g = to_device(ctx, names, seqs)
    try:
        with pytest.raises(NtsError, match=r"record index out of range.*code -22"):
            g.sample_intervals([(0, 0, 10), (len(seqs), 0, 10)], 24, 16)
        with pytest.raises(NtsError, match=r"nts_sample_intervals: bad arguments.*code -22"):
            g.sample_intervals([(0, 0, 100)], 24, 0)
    finally:
        g.free()


def test_two_calls_give_the_same_bytes(ctx):
    names, seqs, iv = genome_end_case(24)
    g = to_device(ctx, names, seqs)
    try:
        a = g.sample_intervals(iv, 24, 16)
        b = g.sample_intervals(iv, 24, 16)
        assert a[0].size > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    finally:
        g.free()

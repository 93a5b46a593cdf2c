"""The lags and their mode (csrc/nts_iv_periods.inc, nts_iv_periods) against the brute force over dictionaries of tests/periods_brute.py:
hand-made lists (a lag held twice, a tie, no recurrence, empty intervals, one hash in two intervals, the extreme hashes and offsets), the
record counts at which the radix sort changes its algorithm, in one interval and over three, 2 * 10^5 random records whose hashes come
from small pools, the empty input, the refused inputs, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests.periods_brute import as_array, brute_periods

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
U64_MAX = (1 << 64) - 1
U32_MAX = (1 << 32) - 1


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


def records(triples):
    "(h0, iv, off) triples as a sampler would return them: by (iv, off)"
    from ntsynt_amd.device import SAMPLE_DTYPE
    out = np.zeros(len(triples), dtype=SAMPLE_DTYPE)
    for i, (h0, iv, off) in enumerate(sorted(triples, key=lambda t: (t[1], t[2]))):
        out[i] = (h0, iv, off)
    return out


def check(ctx, rec, n_iv, what):
    from ntsynt_amd.device import PERIOD_DTYPE
    got = ctx.iv_periods(rec, n_iv)
    exp = as_array(brute_periods([(int(r["h0"]), int(r["iv"]), int(r["off"])) for r in rec], n_iv))
    bad = [i for i in range(n_iv) if got[i].tobytes() != exp[i].tobytes()][:5]
    print(f"{what}: {rec.size} records, {n_iv} intervals, {int((exp['period_hits'] > 0).sum())} with a period; first differences {bad}")
    assert got.dtype == PERIOD_DTYPE and got.shape == (n_iv,), what
    assert not bad, (what, [(i, got[i], exp[i]) for i in bad])
    return got


def test_hand_made_lists(ctx):
    a, b, c = 0x1111, 0x2222, 0x3333
    got = check(ctx, records([(a, 0, 0), (a, 0, 5), (a, 0, 10)]), 1, "one hash at 0, 5, 10")
    assert tuple(got[0]) == (2, 5, 2, 0, 10)
    # lags 3 (a: 0, 3, 6) and 7 (b: 1, 8, 15), two records each: the smaller one
    got = check(ctx, records([(a, 0, 0), (a, 0, 3), (a, 0, 6), (b, 0, 1), (b, 0, 8), (b, 0, 15)]), 1, "a tie of 3 and 7")
    assert tuple(got[0]) == (4, 3, 2, 0, 6)
    # the tie the other way round in offsets: the smaller lag still wins, its extent is its own
    got = check(ctx, records([(a, 0, 20), (a, 0, 27), (a, 0, 34), (b, 0, 41), (b, 0, 44), (b, 0, 47)]), 1, "a tie of 7 and 3")
    assert tuple(got[0]) == (4, 3, 2, 41, 47)
    got = check(ctx, records([(a, 0, 0), (b, 0, 1), (c, 0, 2)]), 1, "records, no recurrence")
    assert tuple(got[0]) == (0, 0, 0, 0, 0)
    got = check(ctx, records([(a, 0, 2), (a, 0, 9), (a, 2, 1), (a, 2, 5), (a, 2, 9)]), 4, "empty intervals in the middle and last")
    assert [tuple(x) for x in got] == [(1, 7, 1, 2, 9), (0, 0, 0, 0, 0), (2, 4, 2, 1, 9), (0, 0, 0, 0, 0)]
    got = check(ctx, records([(a, 0, 10), (a, 1, 20), (b, 1, 30)]), 2, "one hash in two intervals")
    assert not got["recurring"].any()
    got = check(ctx, records([(0, 0, 0), (U64_MAX, 0, 1), (0, 0, 6), (U64_MAX, 0, 7), (0, 0, 12), (U64_MAX, 0, 14)]), 1, "hashes 0 and 2^64 - 1")
    assert tuple(got[0]) == (4, 6, 3, 0, 12)
    got = check(ctx, records([(a, 0, 0), (a, 0, U32_MAX), (b, 1, U32_MAX - 10), (b, 1, U32_MAX - 5), (b, 1, U32_MAX)]), 2, "offsets up to 2^32 - 1")
    assert [tuple(x) for x in got] == [(1, U32_MAX, 1, 0, U32_MAX), (2, 5, 2, U32_MAX - 10, U32_MAX)]
    # a lag's runs of several hashes add up; the extent spans them all
    got = check(ctx, records([(a, 0, 100), (a, 0, 110), (b, 0, 50), (b, 0, 60), (c, 0, 7), (c, 0, 30)]), 1, "one lag from two hashes")
    assert tuple(got[0]) == (3, 10, 2, 50, 110)


def array_like(rng, n, n_iv):
    "n records over n_iv intervals: most of them a tandem array's (a pool of hashes repeating at a period), some noise, some ties"
    triples = []
    share = [n // n_iv + (1 if i < n % n_iv else 0) for i in range(n_iv)]
    for iv, m in enumerate(share):
        period = int(rng.integers(2, 40))
        pool = rng.integers(0, U64_MAX, size=int(rng.integers(1, 6)), dtype=np.uint64, endpoint=True)
        offs = sorted(rng.choice(max(4 * m, 8), size=m, replace=False).tolist())
        for j, off in enumerate(offs):
            h = pool[(off % period) % pool.size] if rng.random() < 0.8 else rng.integers(0, U64_MAX, dtype=np.uint64)
            triples.append((int(h), iv, int(off)))
    return records(triples)


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_sizes_around_the_sorts_change_of_algorithm(ctx, n):
    rng = np.random.default_rng(1400 + n)
    one = check(ctx, array_like(rng, n, 1), 1, f"{n} records in one interval")
    assert int(one[0]["recurring"]) > n // 2                                                   # never a vacuous match
    three = check(ctx, array_like(rng, n, 3), 3, f"{n} records over three intervals")
    assert (three["period_hits"] > 0).all()


@pytest.fixture(scope="module")
def random_records():
    "2 * 10^5 records over 300 intervals, hashes from small pools: most recur and ties occur; (records, brute force), made once"
    from ntsynt_amd.device import SAMPLE_DTYPE
    rng = np.random.default_rng(1414)
    n, n_iv = 200_000, 300
    iv = np.sort(rng.integers(0, n_iv, size=n)).astype(np.uint32)
    iv[iv == 17] = 18                                                                          # an interval without a record
    iv[iv == n_iv - 1] = n_iv - 2                                                              # and the last one
    rec = np.zeros(n, dtype=SAMPLE_DTYPE)
    rec["iv"] = iv
    for i in np.unique(iv):
        at = np.flatnonzero(iv == i)
        rec["off"][at] = np.sort(rng.choice(3 * at.size, size=at.size, replace=False))
        pool = rng.integers(0, U64_MAX, size=int(rng.integers(2, 24)), dtype=np.uint64, endpoint=True)
        rec["h0"][at] = pool[rng.integers(0, pool.size, size=at.size)]
    exp = as_array(brute_periods(zip(rec["h0"].tolist(), rec["iv"].tolist(), rec["off"].tolist()), n_iv))
    return rec, n_iv, exp


def test_random_records_from_small_pools(ctx, random_records):
    rec, n_iv, exp = random_records
    got = ctx.iv_periods(rec, n_iv)
    bad = np.flatnonzero([got[i].tobytes() != exp[i].tobytes() for i in range(n_iv)])[:5]
    recurring = int(exp["recurring"].sum())
    print(f"{rec.size} records, {n_iv} intervals: {recurring} recur, {int((exp['period_hits'] > 0).sum())} intervals with a period; differences {bad}")
    assert recurring > rec.size * 9 // 10 and not exp[17]["recurring"] and not exp[n_iv - 1]["recurring"]
    assert bad.size == 0, [(int(i), got[i], exp[i]) for i in bad]


def test_two_calls_give_the_same_bytes(ctx, random_records):
    rec, n_iv, _ = random_records
    assert ctx.iv_periods(rec, n_iv).tobytes() == ctx.iv_periods(rec, n_iv).tobytes()


def test_no_record_gives_zeros(ctx):
    from ntsynt_amd.device import SAMPLE_DTYPE
    import ctypes
    got = ctx.iv_periods(np.zeros(0, dtype=SAMPLE_DTYPE), 5)
    assert got.shape == (5,) and got.tobytes() == bytes(100)
    out = np.full(25, 0xABABABAB, dtype=np.uint32)                                             # all n_iv entries are written
    assert ctx.lib.nts_iv_periods(ctx.h, None, 0, 5, out.ctypes.data) == 0 and not out.any()
    assert ctx.iv_periods(np.zeros(0, dtype=SAMPLE_DTYPE), 0).size == 0
    assert ctypes.sizeof(ctypes.c_uint32) * 5 == got.dtype.itemsize


def test_errors(ctx):
    from ntsynt_amd.device import NtsError
    a = 0x77
    with pytest.raises(NtsError, match=r"at or beyond n_iv.*code -22"):
        ctx.iv_periods(records([(a, 0, 0), (a, 2, 1)]), 2)
    with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
        rec = records([(a, 0, 0), (a, 1, 1), (a, 2, 2)])
        rec["iv"] = [0, 2, 1]                                                                  # iv decreases
        ctx.iv_periods(rec, 3)
    for offs in ([5, 5], [5, 4]):                                                             # off does not rise
        with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
            rec = records([(a, 0, 0), (a, 0, 1)])
            rec["off"] = offs
            ctx.iv_periods(rec, 1)

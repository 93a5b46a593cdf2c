"""The distinct hashes that carry each interval's period (csrc/nts_iv_families.inc, nts_iv_period_hashes) against the brute force over
dictionaries of tests/families_brute.py: hand-made lists (a lag held twice, another period, a skipped interval, a tie, one hash in two
intervals, empty intervals, the extreme hashes), the record counts at which the radix sort changes its algorithm, in one interval and
over three, 2 * 10^5 random records whose hashes come from small pools with the periods nts_iv_periods finds on the same records, the
empty input, the refused orders, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests.families_brute import as_samples, brute_period_hashes
from tests.periods_brute import brute_periods

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
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


def records(triples):
    "(h0, iv, off) triples as a sampler would return them: by (iv, off)"
    from ntsynt_amd.device import SAMPLE_DTYPE
    out = np.zeros(len(triples), dtype=SAMPLE_DTYPE)
    for i, (h0, iv, off) in enumerate(sorted(triples, key=lambda t: (t[1], t[2]))):
        out[i] = (h0, iv, off)
    return out


def check(ctx, rec, n_iv, period, what):
    from ntsynt_amd.device import SAMPLE_DTYPE
    got = ctx.iv_period_hashes(rec, n_iv, period)
    exp = as_samples(brute_period_hashes(zip(rec["h0"].tolist(), rec["iv"].tolist(), rec["off"].tolist()), n_iv, [int(p) for p in period]))
    print(f"{what}: {rec.size} records, {n_iv} intervals: {exp.size} lines expected, {got.size} returned")
    assert got.dtype == SAMPLE_DTYPE, what
    assert got.tobytes() == exp.tobytes(), (what, got[:8], exp[:8])
    return [(int(r["iv"]), int(r["h0"]), int(r["off"])) for r in got]


def test_hand_made_lists(ctx):
    a, b, c = 0x1111, 0x2222, 0x3333
    assert check(ctx, records([(a, 0, 0), (a, 0, 5), (a, 0, 10)]), 1, [5], "one hash at 0, 5, 10, period 5") == [(0, a, 2)]
    assert check(ctx, records([(a, 0, 0), (a, 0, 5), (a, 0, 10)]), 1, [7], "the same hash, period 7") == []
    assert check(ctx, records([(a, 0, 0), (a, 0, 5), (a, 0, 10)]), 1, [0], "period 0: the interval is skipped") == []
    # lags 3 (a: 0, 3, 6) and 7 (b: 1, 8, 15), two records each: whichever period is named, its hash alone
    tie = records([(a, 0, 0), (a, 0, 3), (a, 0, 6), (b, 0, 1), (b, 0, 8), (b, 0, 15)])
    assert check(ctx, tie, 1, [3], "a tie of 3 and 7, period 3") == [(0, a, 2)]
    assert check(ctx, tie, 1, [7], "a tie of 3 and 7, period 7") == [(0, b, 2)]
    # one hash in two intervals: never paired across them; one line per interval that has the lag
    two = records([(a, 0, 10), (a, 0, 14), (a, 1, 20), (a, 1, 24), (a, 1, 28), (b, 1, 30)])
    assert check(ctx, two, 2, [4, 4], "one hash in two intervals") == [(0, a, 1), (1, a, 2)]
    assert check(ctx, two, 2, [0, 4], "the first of them skipped") == [(1, a, 2)]
    assert check(ctx, records([(a, 0, 10), (a, 1, 14)]), 2, [4, 4], "a lag across two intervals is none") == []
    mid = records([(a, 0, 2), (a, 0, 9), (a, 2, 1), (a, 2, 5), (a, 2, 9)])
    assert check(ctx, mid, 4, [7, 3, 4, 9], "empty intervals in the middle and last") == [(0, a, 1), (2, a, 2)]
    ends = records([(0, 0, 0), (U64_MAX, 0, 1), (0, 0, 6), (U64_MAX, 0, 7), (0, 0, 12), (U64_MAX, 0, 14)])
    assert check(ctx, ends, 1, [6], "hashes 0 and 2^64 - 1") == [(0, 0, 2), (0, U64_MAX, 1)]
    # two hashes at one lag, a third at another: sorted by hash within the interval, the count per hash
    mix = records([(c, 0, 100), (c, 0, 110), (c, 0, 120), (a, 0, 50), (a, 0, 60), (b, 0, 7), (b, 0, 30)])
    assert check(ctx, mix, 1, [10], "one lag from two hashes") == [(0, a, 1), (0, c, 2)]


def array_like(rng, n, n_iv):
    """n records over n_iv intervals, most of them a tandem array's (a pool of hashes repeating at a period); (records, per interval the
    lag most records hold, by the brute force of tests/periods_brute.py)"""
    triples = []
    share = [n // n_iv + (1 if i < n % n_iv else 0) for i in range(n_iv)]
    for iv, m in enumerate(share):
        period = int(rng.integers(2, 40))
        pool = rng.integers(0, U64_MAX, size=int(rng.integers(1, 6)), dtype=np.uint64, endpoint=True)
        for off in sorted(rng.choice(max(4 * m, 8), size=m, replace=False).tolist()):
            h = pool[(off % period) % pool.size] if rng.random() < 0.8 else rng.integers(0, U64_MAX, dtype=np.uint64)
            triples.append((int(h), iv, int(off)))
    return records(triples), [r[1] for r in brute_periods(triples, n_iv)]


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_sizes_around_the_sorts_change_of_algorithm(ctx, n):
    rng = np.random.default_rng(1500 + n)
    rec, periods = array_like(rng, n, 1)
    assert check(ctx, rec, 1, periods, f"{n} records in one interval")                         # never a vacuous match
    rec, periods = array_like(rng, n, 3)
    assert {iv for iv, _, _ in check(ctx, rec, 3, periods, f"{n} records over three intervals")} == {0, 1, 2}


@pytest.fixture(scope="module")
def random_records(ctx):
    "2 * 10^5 records over 300 intervals, hashes from small pools; the periods are nts_iv_periods' on the same records; made once"
    from ntsynt_amd.device import SAMPLE_DTYPE
    rng = np.random.default_rng(1515)
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
    period = ctx.iv_periods(rec, n_iv)["period"].copy()
    period[5] = 0                                                                              # one interval skipped
    exp = as_samples(brute_period_hashes(zip(rec["h0"].tolist(), rec["iv"].tolist(), rec["off"].tolist()), n_iv, period.tolist()))
    return rec, n_iv, period, exp


def test_random_records_from_small_pools(ctx, random_records):
    rec, n_iv, period, exp = random_records
    got = ctx.iv_period_hashes(rec, n_iv, period)
    print(f"{rec.size} records, {n_iv} intervals: {exp.size} lines expected, {got.size} returned, {int(exp['off'].sum())} records at their period")
    assert exp.size > 1000 and not (exp["iv"] == 5).any() and not (exp["iv"] == 17).any() and (np.diff(exp["iv"].astype(np.int64)) >= 0).all()
    assert got.tobytes() == exp.tobytes()


def test_two_calls_give_the_same_bytes(ctx, random_records):
    rec, n_iv, period, _ = random_records
    assert ctx.iv_period_hashes(rec, n_iv, period).tobytes() == ctx.iv_period_hashes(rec, n_iv, period).tobytes()


def test_no_record_gives_nothing(ctx):
    from ntsynt_amd.device import SAMPLE_DTYPE
    assert ctx.iv_period_hashes(np.zeros(0, dtype=SAMPLE_DTYPE), 5, [3] * 5).size == 0
    assert ctx.iv_period_hashes(np.zeros(0, dtype=SAMPLE_DTYPE), 0, []).size == 0
    assert ctx.iv_period_hashes(records([(1, 0, 0), (1, 0, 4)]), 1, [0]).size == 0


def test_errors(ctx):
    from ntsynt_amd.device import NtsError
    a = 0x77
    with pytest.raises(NtsError, match=r"nts_iv_period_hashes.*at or beyond n_iv.*code -22"):
        ctx.iv_period_hashes(records([(a, 0, 0), (a, 2, 1)]), 2, [1, 1])
    with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
        rec = records([(a, 0, 0), (a, 1, 1), (a, 2, 2)])
        rec["iv"] = [0, 2, 1]                                                                  # iv decreases
        ctx.iv_period_hashes(rec, 3, [1, 1, 1])
    for offs in ([5, 5], [5, 4]):                                                             # off does not rise
        with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
            rec = records([(a, 0, 0), (a, 0, 1)])
            rec["off"] = offs
            ctx.iv_period_hashes(rec, 1, [1])
    with pytest.raises(ValueError, match="one period per interval"):
        ctx.iv_period_hashes(records([(a, 0, 0)]), 2, [1])

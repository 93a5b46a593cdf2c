"""The anchor join and the segments (csrc/nts_iv_anchors.inc, nts_iv_anchor_segments) against the dictionaries of
tests/identity_brute.py: a hash twice in a list, a hash in intervals that are not mates, no mate, the mirroring of a flipped pair at
both ends of the interval, y falling and standing still, dx and |dy - dx| at and just beyond their limits, a single anchor, the
extreme hashes, the record counts at which the radix sort changes its algorithm, 2 * 10^5 random records over 300 interval pairs, empty
lists, lists out of sampler order, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
U64_MAX = (1 << 64) - 1
K = 21


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
    for i, t in enumerate(sorted(triples, key=lambda t: (t[1], t[2]))):
        out[i] = t
    return out


def check(ctx, a, b, mate, len_b, flip, what, k=K, band=31, max_len=4096):
    from ntsynt_amd.device import SEGMENT_DTYPE
    ra, rb = records(a), records(b)
    got, per_iv = ctx.iv_anchor_segments(ra, rb, mate, len_b, flip, k, band, max_len)
    again, per_again = ctx.iv_anchor_segments(ra, rb, mate, len_b, flip, k, band, max_len)
    exp, exp_iv = B.brute_segments(a, b, mate, len_b, flip, k, band, max_len)
    print(f"{what}: {len(a)} + {len(b)} records, {len(mate)} intervals, {sum(exp_iv)} anchors, {len(exp)} segments")
    assert got.dtype == SEGMENT_DTYPE
    assert [tuple(int(v) for v in s) for s in got] == exp, what
    assert per_iv.tolist() == exp_iv, what
    assert got.tobytes() == again.tobytes() and per_iv.tobytes() == per_again.tobytes(), what
    return exp, exp_iv


def test_what_is_an_anchor(ctx):
    h = list(range(0x100, 0x120))
    # a hash twice in A's list, once in another interval of A: no anchor for any pair
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, 10), (h[2], 0, 20), (h[1], 1, 5)], [(h[0], 0, 0), (h[1], 0, 10), (h[2], 0, 20)], [0, 1], [100, 100],
                     [0, 0], "a hash twice in A")
    assert per == [2, 0] and exp == [(0, 0, 20, 0, 20, B.CANDIDATE)]
    # once in each list, in intervals that are not mates
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, 10), (h[2], 1, 0), (h[3], 1, 10)], [(h[0], 1, 0), (h[1], 1, 10), (h[2], 1, 0 + 30), (h[3], 1, 40)],
                     [0, 1], [100, 100], [0, 0], "not mates")
    assert per == [0, 2]
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, 10)], [(h[0], 0, 0), (h[1], 0, 10)], [B.NO_MATE], [100], [0], "no mate")
    assert per == [0] and exp == []
    exp, per = check(ctx, [(h[0], 0, 7)], [(h[0], 0, 7)], [0], [100], [0], "a single anchor")
    assert per == [1] and exp == []
    exp, per = check(ctx, [(0, 0, 0), (U64_MAX, 0, 9)], [(0, 0, 3), (U64_MAX, 0, 12)], [0], [100], [0], "hashes 0 and 2^64 - 1")
    assert exp == [(0, 0, 9, 3, 9, B.CANDIDATE)]
    # a hash twice in B
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, 10), (h[2], 0, 20)], [(h[0], 0, 0), (h[1], 0, 10), (h[1], 0, 11), (h[2], 0, 20)], [0], [100], [0],
                     "a hash twice in B")
    assert per == [2]


def test_flip_and_kinds(ctx):
    h = list(range(0x200, 0x240))
    lb = 500
    # off_b = L_b - k mirrors to y = 0, off_b = 0 to y = L_b - k
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, lb - K)], [(h[1], 0, 0), (h[0], 0, lb - K)], [0], [lb], [1], "mirroring at both ends")
    assert exp == [(0, 0, lb - K, 0, lb - K, B.CANDIDATE)]
    # y falling, y standing still (a flipped pair gives two records of B one y only through different lengths: use a forward pair)
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 0, 10), (h[2], 0, 20)], [(h[0], 0, 50), (h[1], 0, 40), (h[2], 0, 60)], [0], [lb], [0], "y falls")
    assert [s[5] for s in exp] == [B.BACKWARD, B.CANDIDATE]
    exp, per = check(ctx, [(h[0], 0, 0), (h[1], 1, 10), (h[2], 1, 30)], [(h[1], 0, 40), (h[2], 1, 40)], [0, 0], [lb, lb], [0, 0], "two intervals of A, one mate")
    assert per == [0, 1]
    for max_len, kinds in ((100, [B.CANDIDATE]), (99, [B.LONG])):
        exp, _ = check(ctx, [(h[0], 0, 0), (h[1], 0, 100)], [(h[0], 0, 0), (h[1], 0, 100)], [0], [lb], [0], f"dx 100 against max_len {max_len}",
                       max_len=max_len)
        assert [s[5] for s in exp] == kinds
    for band, dy, kinds in ((7, 107, [B.CANDIDATE]), (7, 108, [B.OFFBAND]), (7, 93, [B.CANDIDATE]), (7, 92, [B.OFFBAND]), (31, 131, [B.CANDIDATE]),
                            (31, 132, [B.OFFBAND]), (1, 101, [B.CANDIDATE]), (1, 102, [B.OFFBAND])):
        exp, _ = check(ctx, [(h[0], 0, 0), (h[1], 0, 100)], [(h[0], 0, 0), (h[1], 0, dy)], [0], [lb], [0], f"dy - dx {dy - 100} in band {band}", band=band)
        assert [s[5] for s in exp] == kinds


def random_lists(rng, n_each, n_pairs):
    """two lists over n_pairs interval pairs.  A's hashes come from a pool that makes some occur twice; six in ten of A's records are
    repeated in the mate of their interval, near their own offset (mirrored where the pair is flipped) -- most in order, some not, some
    far off the diagonal --, and B is filled up to A's size with the pool's hashes, in any interval"""
    span = 20000
    pool = rng.integers(0, 1 << 63, size=n_each, dtype=np.uint64)
    hs = pool[rng.integers(0, n_each, size=n_each)]
    iv = np.sort(rng.integers(0, n_pairs, size=n_each))
    off = np.zeros(n_each, dtype=np.int64)
    for v in np.unique(iv):
        m = iv == v
        off[m] = np.sort(rng.choice(span, size=int(m.sum()), replace=False))
    a = [(int(x), int(y), int(z)) for x, y, z in zip(hs, iv, off)]
    mate = rng.permutation(n_pairs).astype(np.int64)
    mate[rng.random(n_pairs) < 0.05] = B.NO_MATE
    flip = (rng.random(n_pairs) < 0.3).astype(int)
    taken = {}
    for h, v, o in a:
        if mate[v] == B.NO_MATE or rng.random() >= 0.6:
            continue
        y = o + int(rng.integers(-60, 61)) + (int(rng.integers(-5000, 5000)) if rng.random() < 0.02 else 0)
        y = min(max(y, 0), span - 1)
        taken.setdefault((int(mate[v]), span - 1 - y if flip[v] else y), h)
    while len(taken) < n_each:
        taken.setdefault((int(rng.integers(0, n_pairs)), int(rng.integers(0, span))), int(pool[rng.integers(0, n_each)]))
    b = [(h, v, o) for (v, o), h in taken.items()]
    return a, b, mate.tolist(), [span - 1 + K] * n_pairs, flip.tolist()


@pytest.mark.parametrize("n_each", [255, 256, 257, 1024, 1025])
def test_sort_thresholds(ctx, n_each):
    a, b, mate, len_b, flip = random_lists(np.random.default_rng(n_each), n_each, 3)
    exp, per = check(ctx, a, b[:n_each], mate, len_b, flip, f"{n_each} records each")
    assert sum(per) > 0 and len(a) == n_each and len(b) >= n_each


def test_random_records(ctx):
    a, b, mate, len_b, flip = random_lists(np.random.default_rng(7), 100_000, 300)
    exp, per = check(ctx, a, b[:100_000], mate, len_b, flip, "2 * 10^5 random records")
    kinds = {s[5] for s in exp}
    print("kinds seen:", sorted(kinds), "anchors", sum(per))
    assert kinds == {B.CANDIDATE, B.BACKWARD, B.LONG, B.OFFBAND} and sum(per) > 10_000


def test_empty_and_refused(ctx):
    from ntsynt_amd.device import NtsError
    exp, per = check(ctx, [], [], [0, B.NO_MATE], [10, 10], [0, 0], "empty lists")
    assert per == [0, 0] and exp == []
    exp, per = check(ctx, [(5, 0, 0)], [], [0], [10], [0], "an empty B")
    exp, per = check(ctx, [], [], [], [], [], "no interval")
    good = records([(1, 0, 0), (2, 0, 5)])

    def refused(a, b, mate=(0,), len_b=(100,), flip=(0,), k=K, band=31, max_len=4096):
        with pytest.raises(NtsError) as err:
            ctx.iv_anchor_segments(a, b, list(mate), list(len_b), list(flip), k, band, max_len)
        assert "code -22" in str(err.value), err.value
    refused(good[::-1].copy(), good)                          # out of sampler order
    refused(good, good[::-1].copy())
    refused(records([(1, 0, 0), (2, 0, 0)]), good)            # off does not rise
    refused(records([(1, 1, 0)]), good)                       # iv >= n_iv_a
    refused(good, good, flip=(2,))
    for kw in (dict(k=0), dict(band=0), dict(band=32), dict(max_len=0), dict(max_len=65536)):
        refused(good, good, **kw)

"""The arrays that share a hash joined into families (csrc/nts_iv_families.inc, nts_iv_families) against the brute union-find of
tests/families_brute.py: a chain joined through two different hashes, disjoint groups, an array without a pair, one hash in three
arrays, duplicate pairs, the extreme hashes, the joining pair last, 2 * 10^5 random pairs over 3 000 arrays from small pools, the empty
input, an array index beyond n_arrays, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests.families_brute import brute_families

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


def pairs_of(pairs, off=0):
    "(h0, array) pairs in the given order as records; off is ignored by the call"
    from ntsynt_amd.device import SAMPLE_DTYPE
    out = np.zeros(len(pairs), dtype=SAMPLE_DTYPE)
    for i, (h0, a) in enumerate(pairs):
        out[i] = (h0, a, off)
    return out


def check(ctx, pairs, n_arrays, what):
    family, hashes, hash_family = ctx.iv_families(pairs_of(pairs, off=len(pairs)), n_arrays)
    exp = brute_families(pairs, n_arrays)
    print(f"{what}: {len(pairs)} pairs, {n_arrays} arrays: {len(set(exp[0]))} families, {len(exp[1])} hashes")
    assert (family.dtype, hashes.dtype, hash_family.dtype) == (np.uint32, np.uint64, np.uint32), what
    assert family.tolist() == exp[0], what
    assert hashes.tolist() == exp[1], what
    assert hash_family.tolist() == exp[2], what
    return family.tolist(), hashes.tolist(), hash_family.tolist()


def test_hand_made_pairs(ctx):
    x, y, z = 0x10, 0x20, 0x30
    # a - b through x, b - c through y: one family although a and c share nothing
    assert check(ctx, [(x, 0), (x, 1), (y, 1), (y, 2)], 3, "a chain through two hashes") == ([0, 0, 0], [x, y], [0, 0])
    assert check(ctx, [(x, 0), (x, 2), (y, 1), (y, 3)], 4, "two disjoint groups") == ([0, 1, 0, 1], [x, y], [0, 1])
    assert check(ctx, [(x, 0), (x, 2)], 4, "arrays without a pair") == ([0, 1, 0, 3], [x], [0])
    assert check(ctx, [(x, 3), (x, 1), (x, 2), (y, 0)], 4, "one hash in three arrays") == ([0, 1, 1, 1], [x, y], [1, 0])
    assert check(ctx, [(x, 1), (x, 1), (x, 0), (x, 1), (x, 0), (y, 2), (y, 2)], 3, "duplicate pairs") == ([0, 0, 2], [x, y], [0, 2])
    assert check(ctx, [(0, 1), (U64_MAX, 2), (0, 3), (U64_MAX, 0)], 4, "hashes 0 and 2^64 - 1") == ([0, 1, 0, 1], [0, U64_MAX], [1, 0])
    # 3 - 4 and 1 - 2 first, then 2 - 3, and the pair that brings in array 0 last: the smallest index wins all the same
    late = [(x, 3), (x, 4), (y, 1), (y, 2), (z, 2), (z, 3), (0x40, 4), (0x40, 0)]
    assert check(ctx, late, 5, "the joining pair comes last") == ([0, 0, 0, 0, 0], [x, y, z, 0x40], [0, 0, 0, 0])
    assert check(ctx, [(x, 0)], 1, "one pair") == ([0], [x], [0])


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_sizes_around_the_sorts_change_of_algorithm(ctx, n):
    rng = np.random.default_rng(1600 + n)
    pool = rng.integers(0, U64_MAX, size=n // 3, dtype=np.uint64, endpoint=True)
    pairs = [(int(pool[rng.integers(0, pool.size)]), int(rng.integers(0, n // 4))) for _ in range(n)]
    family, _, _ = check(ctx, pairs, n // 4, f"{n} pairs")
    assert 1 < len(set(family)) < n // 4                                                       # joined, and not all into one


@pytest.fixture(scope="module")
def random_pairs():
    "2 * 10^5 pairs over 3 000 arrays: every group of 30 arrays draws from a pool of its own, some hashes join two groups; made once"
    rng = np.random.default_rng(1616)
    n, n_arrays, group = 200_000, 3_000, 30
    a = rng.integers(0, n_arrays, size=n)
    a[a == 1234] = 1235                                                                        # an array without a pair
    pools = rng.integers(0, U64_MAX, size=(n_arrays // group, 40), dtype=np.uint64, endpoint=True)
    g = a // group
    bridge = (rng.random(n) < 0.0002) & (g % 3 == 0) & (g + 1 < n_arrays // group)              # a hash of the next group's pool
    h = pools[np.where(bridge, g + 1, g), rng.integers(0, 40, size=n)]
    pairs = list(zip(h.tolist(), a.tolist()))
    return pairs, n_arrays, brute_families(pairs, n_arrays)


def test_random_pairs_from_small_pools(ctx, random_pairs):
    pairs, n_arrays, exp = random_pairs
    family, hashes, hash_family = ctx.iv_families(pairs_of(pairs), n_arrays)
    sizes = np.bincount(np.asarray(exp[0]))
    print(f"{len(pairs)} pairs, {n_arrays} arrays: {int((sizes > 0).sum())} families, the largest of {int(sizes.max())}, {len(exp[1])} hashes")
    assert exp[0][1234] == 1234 and 60 in sizes and 30 in sizes and 1 in sizes                # bridged groups, plain ones and the lone array
    assert family.tolist() == exp[0]
    assert hashes.tolist() == exp[1]
    assert hash_family.tolist() == exp[2]


def test_two_calls_give_the_same_bytes(ctx, random_pairs):
    pairs, n_arrays, _ = random_pairs
    rec = pairs_of(pairs)
    one, two = ctx.iv_families(rec, n_arrays), ctx.iv_families(rec, n_arrays)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))


def test_no_pair_gives_every_array_itself(ctx):
    family, hashes, hash_family = ctx.iv_families(pairs_of([]), 4)
    assert family.tolist() == [0, 1, 2, 3] and hashes.size == 0 and hash_family.size == 0
    family, hashes, hash_family = ctx.iv_families(pairs_of([]), 0)
    assert family.size == 0 and hashes.size == 0 and hash_family.size == 0


def test_errors(ctx):
    from ntsynt_amd.device import NtsError
    with pytest.raises(NtsError, match=r"nts_iv_families.*at or beyond n_arrays.*code -22"):
        ctx.iv_families(pairs_of([(1, 0), (1, 2)]), 2)
    with pytest.raises(NtsError, match=r"at or beyond n_arrays.*code -22"):
        ctx.iv_families(pairs_of([(1, 0)]), 0)

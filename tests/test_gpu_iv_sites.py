"""The join of gap copy sites (csrc/nts_iv_sites.inc, nts_iv_sites) against a brute force over dictionaries that restates the
definitions (tests/sites_brute.py): hand-made lists, the pair writer's edges, random input with multiplicity on both sides, empty
input, determinism.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests.sites_brute import brute_sites, samples

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600


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


def check(ctx, lists, target, step, min_hits, what):
    "the device's sites against the brute force, field for field and in order; returns them as tuples"
    from ntsynt_amd.device import SITE_DTYPE
    got = ctx.iv_sites(lists, target, step, min_hits)
    exp = brute_sites(lists, target, step, min_hits)
    assert got.dtype == SITE_DTYPE
    rows = [tuple(int(x) for x in r) for r in got]
    print(f"{what}: {sum(len(a) for a in lists)} query records, {len(target)} target records, step {step}, min_hits {min_hits}: {len(rows)} sites")
    assert rows == exp, (what, rows[:5], exp[:5])
    return rows


def test_hand_made_lists(ctx):
    # one query record with many targets: positions 0, 10, ..., 90 of record 0, then 500 of record 0 and 5 of record 1
    many = samples([(7, 0, 3)])
    tgt = samples([(7, 0, 10 * i) for i in range(10)] + [(7, 0, 500), (7, 1, 5)])
    assert check(ctx, [many], tgt, 10, 1, "one query, many targets") == [(0, 0, 0, 10, 0, 0, 3, 3, 0, 90), (0, 0, 0, 1, 0, 0, 3, 3, 500, 500),
                                                                         (0, 0, 1, 1, 0, 0, 3, 3, 5, 5)]
    assert check(ctx, [many], tgt, 9, 1, "one query, many targets, every one its own site") == \
        [(0, 0, 0, 1, 0, 0, 3, 3, 10 * i, 10 * i) for i in range(10)] + [(0, 0, 0, 1, 0, 0, 3, 3, 500, 500), (0, 0, 1, 1, 0, 0, 3, 3, 5, 5)]
    # one hash twice in a gap and three times in the target: six pairs; at one position the two records stay in query order (40 then 20: a fall)
    twice = samples([(9, 0, 40), (9, 0, 20)])
    thrice = samples([(9, 2, 100), (9, 2, 150), (9, 2, 200)])
    assert check(ctx, [twice], thrice, 50, 1, "two by three") == [(0, 0, 2, 6, 2, 3, 20, 40, 100, 200)]       # 40 20 | 40 20 | 40 20: three falls, two rises
    assert check(ctx, [twice], thrice, 49, 1, "two by three, three sites") == [(0, 0, 2, 2, 0, 1, 20, 40, p, p) for p in (100, 150, 200)]
    # a site broken exactly at step and at step + 1
    q = samples([(1, 0, 0), (2, 0, 10), (3, 0, 20)])
    t = samples([(1, 0, 1000), (2, 0, 1100), (3, 0, 1201)])
    assert check(ctx, [q], t, 100, 1, "gaps of step and step + 1") == [(0, 0, 0, 2, 1, 0, 0, 10, 1000, 1100), (0, 0, 0, 1, 0, 0, 20, 20, 1201, 1201)]
    assert check(ctx, [q], t, 101, 1, "step + 1 closes it") == [(0, 0, 0, 3, 2, 0, 0, 20, 1000, 1201)]
    # step 0: only pairs at one position share a site
    t0 = samples([(1, 0, 77), (2, 0, 77), (3, 0, 78)])
    assert check(ctx, [q], t0, 0, 1, "step 0") == [(0, 0, 0, 2, 1, 0, 0, 10, 77, 77), (0, 0, 0, 1, 0, 0, 20, 20, 78, 78)]
    # two records of the target at the same position in different rec: never one site
    t2 = samples([(1, 0, 500), (2, 1, 500), (3, 1, 500)])
    assert check(ctx, [q], t2, 1000, 1, "one position, two records") == [(0, 0, 0, 1, 0, 0, 0, 0, 500, 500), (0, 0, 1, 2, 1, 0, 10, 20, 500, 500)]
    # min_hits 1 and 4; two gaps of one list and a second list, a reversed copy (offsets fall as positions rise)
    a = samples([(10 + i, 0, 5 * i) for i in range(5)] + [(20 + i, 1, 7 * i) for i in range(3)])
    b = samples([(10 + i, 0, 100 - 9 * i) for i in range(4)])
    tg = samples([(10 + i, 3, 1000 + 30 * i) for i in range(5)] + [(10 + i, 3, 9000 - 30 * i) for i in range(5)] + [(20 + i, 0, 50 * i) for i in range(3)])
    one = check(ctx, [a, b], tg, 30, 1, "min_hits 1")
    four = check(ctx, [a, b], tg, 30, 4, "min_hits 4")
    assert len(one) == 7 and four == [r for r in one if r[3] >= 4] and len(four) == 4
    assert (0, 0, 3, 5, 4, 0, 0, 20, 1000, 1120) in four and (0, 0, 3, 5, 0, 4, 0, 20, 8880, 9000) in four and (1, 0, 3, 4, 0, 3, 73, 100, 1000, 1090) in four
    # pairs whose offsets are equal: neither fwd nor rev
    same = samples([(1, 0, 5), (2, 0, 5), (3, 0, 5)])
    assert check(ctx, [same], t, 1000, 1, "equal offsets") == [(0, 0, 0, 3, 0, 0, 5, 5, 1000, 1201)]


@pytest.mark.parametrize("n_pairs", [255, 256, 257, 1025])
def test_the_pair_writer_at_the_edges_of_a_workgroup(ctx, n_pairs):
    """n_pairs pairs in all; query records without a match first, last and in a run of several hundred in the middle: a pair's lane finds
    its query record by an upper bound in the scan of the counts, and the records without a match share a scan value with their successor"""
    rng = np.random.default_rng(n_pairs)
    mult = []                                                                   # target multiplicity per matching query record, 1..4, summing to n_pairs
    while sum(mult) < n_pairs:
        mult.append(min(int(rng.integers(1, 5)), n_pairs - sum(mult)))
    half = len(mult) // 2
    target, rows, pos = [], [], 0
    miss = iter(range(10**6, 2 * 10**6))
    rows += [(next(miss), 0, 3 * j) for j in range(5)]                          # no match first
    for i, m in enumerate(mult):
        if i == half:
            rows += [(next(miss), 0, 7000 + j) for j in range(300)]             # several hundred without a match in the middle
        rows.append((1000 + i, i % 3, 10 * i))
        for _ in range(m):
            target.append((1000 + i, int(rng.integers(0, 2)), pos))
            pos += int(rng.integers(0, 40))
    rows += [(next(miss), 2, 9 * j) for j in range(4)]                          # and last
    target = [target[j] for j in rng.permutation(len(target))]
    lists, tgt = [samples(rows)], samples(target)
    assert sum(int((tgt["h0"] == np.uint64(h)).sum()) for h, _, _ in rows) == n_pairs
    for step, min_hits in ((20, 1), (45, 2)):
        got = check(ctx, lists, tgt, step, min_hits, f"{n_pairs} pairs")
        if min_hits == 1:
            assert sum(r[3] for r in got) == n_pairs                           # every pair lies in exactly one site


def test_random_lists_with_multiplicity_on_both_sides(ctx):
    rng = np.random.default_rng(4130)
    pool = rng.integers(0, 1 << 62, size=60_000, dtype=np.uint64)
    n_t = 200_000
    lists = []
    for n, gaps in ((90_000, 40), (0, 1), (110_000, 25)):                      # three lists, the middle one empty
        part = np.zeros(n, dtype=samples([]).dtype)
        part["h0"] = pool[rng.integers(0, pool.size, size=n)]
        part["iv"] = np.sort(rng.integers(0, gaps, size=n)).astype(np.uint32)
        part["off"] = rng.integers(0, 6_000, size=n).astype(np.uint32)
        lists.append(part)
    tgt = np.zeros(n_t, dtype=lists[0].dtype)
    tgt["h0"] = pool[rng.integers(0, pool.size, size=n_t)]
    tgt["iv"] = rng.integers(0, 5, size=n_t).astype(np.uint32)
    tgt["off"] = rng.integers(0, 3_000_000, size=n_t).astype(np.uint32)
    for side in (np.concatenate([a["h0"] for a in lists]), tgt["h0"]):
        seen = set(int(x) for x in np.unique(side, return_counts=True)[1])
        assert set(range(1, 9)) <= seen, seen                                   # multiplicities 1..8 on both sides
    # about 10^4 pairs per gap over 5 records of 3 Mbp: neighbours some 1 500 bases apart -- at this step sites of one and of many pairs
    got = check(ctx, lists, tgt, 1500, 1, "random")
    sizes = np.array([r[3] for r in got])
    print(f"{sizes.size} sites, {int(sizes.sum())} pairs, largest {int(sizes.max())}, singletons {int((sizes == 1).sum())}")
    assert int((sizes == 1).sum()) > 1000 and int((sizes >= 8).sum()) > 1000 and {0, 2} == {r[0] for r in got}
    kept = ctx.iv_sites(lists, tgt, 1500, 4)                                    # the selection: what the brute force has with four pairs or more
    assert [tuple(int(x) for x in r) for r in kept] == [r for r in got if r[3] >= 4] and 0 < kept.size < len(got)
    assert kept.tobytes() == ctx.iv_sites(lists, tgt, 1500, 4).tobytes()        # determinism: two calls give the same bytes


def test_empty_input(ctx):
    q = samples([(1, 0, 0), (2, 0, 10)])
    t = samples([(1, 0, 5), (2, 0, 6)])
    assert ctx.iv_sites([q], t, 10, 1).size == 1
    assert ctx.iv_sites([q], samples([]), 10, 1).size == 0                      # an empty target
    assert ctx.iv_sites([samples([])], t, 10, 1).size == 0                      # an empty list
    assert ctx.iv_sites([], t, 10, 1).size == 0                                 # no list
    assert ctx.iv_sites([q], samples([(3, 0, 5)]), 10, 1).size == 0             # and no hash in common
    from ntsynt_amd.device import NtsError
    with pytest.raises(NtsError, match="nts_iv_sites: bad arguments"):
        ctx.iv_sites([q], t, 10, 0)

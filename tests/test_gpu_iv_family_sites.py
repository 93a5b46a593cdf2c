"""One genome's occurrences of the families' hashes grouped into sites (csrc/nts_iv_families.inc, nts_iv_family_sites) against the brute
force of tests/families_brute.py: consecutive offsets exactly step and step + 1 apart, a change of record inside a run, two families
interleaved over one stretch, min_hits at and one below a site's hits, a hash that is not in the table, offsets up to 2^32 - 1, the
occurrence counts at which the radix sort changes its algorithm, 2 * 10^5 random occurrences over 40 records and 50 families, the empty
inputs, the refused inputs, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests.families_brute import as_sites, brute_family_sites

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


def occurrences(triples):
    "(h0, rec, pos) triples as a sweep over whole records returns them: by (rec, pos)"
    from ntsynt_amd.device import SAMPLE_DTYPE
    out = np.zeros(len(triples), dtype=SAMPLE_DTYPE)
    for i, (h0, rec, pos) in enumerate(sorted(triples, key=lambda t: (t[1], t[2]))):
        out[i] = (h0, rec, pos)
    return out


def check(ctx, occ, family_of, step, min_hits, what):
    from ntsynt_amd.device import FSITE_DTYPE
    hashes = np.array(sorted(family_of), dtype=np.uint64)
    hash_family = np.array([family_of[h] for h in sorted(family_of)], dtype=np.uint32)
    got = ctx.iv_family_sites(occ, hashes, hash_family, step, min_hits)
    exp = as_sites(brute_family_sites(zip(occ["h0"].tolist(), occ["iv"].tolist(), occ["off"].tolist()), family_of, step, min_hits))
    print(f"{what}: {occ.size} occurrences, {hashes.size} hashes, step {step}, min_hits {min_hits}: {exp.size} sites expected, {got.size} returned")
    assert got.dtype == FSITE_DTYPE, what
    assert got.tobytes() == exp.tobytes(), (what, got[:8], exp[:8])
    return [tuple(int(x) for x in s) for s in got]


def test_hand_made_occurrences(ctx):
    a, b, c = 0x1111, 0x2222, 0x3333
    one = {a: 1}
    # 0, 10, 20: exactly step apart -- one site; 0, 10, 21: the last is step + 1 away and alone
    assert check(ctx, occurrences([(a, 0, 0), (a, 0, 10), (a, 0, 20)]), one, 10, 1, "exactly step apart") == [(1, 0, 0, 20, 3)]
    assert check(ctx, occurrences([(a, 0, 0), (a, 0, 10), (a, 0, 21)]), one, 10, 1, "step + 1 apart") == [(1, 0, 0, 10, 2), (1, 0, 21, 21, 1)]
    assert check(ctx, occurrences([(a, 0, 0), (a, 0, 0 + 1)]), one, 0, 1, "step 0") == [(1, 0, 0, 0, 1), (1, 0, 1, 1, 1)]
    # the record changes inside what the positions alone would call a run
    assert check(ctx, occurrences([(a, 0, 100), (a, 0, 105), (a, 1, 107), (a, 1, 109)]), one, 10, 1, "a change of record") == \
        [(1, 0, 100, 105, 2), (1, 1, 107, 109, 2)]
    # two families interleaved over one stretch: each is a site of its own, neither breaks the other (4 apart, step 5)
    two = {a: 1, b: 2}
    inter = occurrences([(a, 0, 0), (b, 0, 2), (a, 0, 4), (b, 0, 6), (a, 0, 8), (b, 0, 10)])
    assert check(ctx, inter, two, 5, 3, "two families interleaved") == [(1, 0, 0, 8, 3), (2, 0, 2, 10, 3)]
    assert check(ctx, inter, {a: 7, b: 7}, 5, 3, "the same stretch, one family of two hashes") == [(7, 0, 0, 10, 6)]
    # min_hits at, and one above, a site's hits
    runs = occurrences([(a, 0, 0), (a, 0, 1), (a, 0, 2), (a, 0, 100), (a, 0, 101)])
    assert check(ctx, runs, one, 5, 3, "min_hits at a site's hits") == [(1, 0, 0, 2, 3)]
    assert check(ctx, runs, one, 5, 2, "min_hits one below") == [(1, 0, 0, 2, 3), (1, 0, 100, 101, 2)]
    assert check(ctx, runs, one, 5, 4, "min_hits one above") == []
    # a hash that is not in the table is dropped and breaks nothing; hashes below, between and above the table's
    stray = occurrences([(a, 0, 0), (c, 0, 1), (a, 0, 2), (5, 0, 3), (U64_MAX, 0, 4), (0x2000, 0, 5), (b, 0, 6)])
    assert check(ctx, stray, two, 5, 1, "a hash that is not in the table") == [(1, 0, 0, 2, 2), (2, 0, 6, 6, 1)]
    assert check(ctx, stray, {c + 1: 1}, 5, 1, "no occurrence is a member") == []
    ends = {0: 3, U64_MAX: 4}
    far = occurrences([(0, 0, 0), (U64_MAX, 0, 1), (0, 2, U32_MAX - 10), (0, 2, U32_MAX), (U64_MAX, 2, U32_MAX - 1), (0, 0, U32_MAX)])
    assert check(ctx, far, ends, 10, 1, "offsets up to 2^32 - 1, hashes 0 and 2^64 - 1, family ids out of order") == \
        [(3, 0, 0, 0, 1), (3, 0, U32_MAX, U32_MAX, 1), (3, 2, U32_MAX - 10, U32_MAX, 2), (4, 0, 1, 1, 1), (4, 2, U32_MAX - 1, U32_MAX - 1, 1)]
    assert check(ctx, far, ends, U32_MAX, 2, "step 2^32 - 1") == [(3, 0, 0, U32_MAX, 2), (3, 2, U32_MAX - 10, U32_MAX, 2)]
    assert check(ctx, occurrences([(a, 0, 0), (a, 0, 3)]), {a: U32_MAX}, 5, 1, "family 2^32 - 1") == [(U32_MAX, 0, 0, 3, 2)]


def random_occurrences(rng, n, n_rec, n_fam, span):
    "(occurrences, family_of): n distinct (rec, pos) over n_rec records of `span` bases; one hash in five is no member"
    from ntsynt_amd.device import SAMPLE_DTYPE
    pool = np.unique(rng.integers(0, U64_MAX, size=6 * n_fam, dtype=np.uint64, endpoint=True))
    members = pool[: pool.size * 4 // 5]
    family_of = {int(h): int(f) + 1 for h, f in zip(members, rng.permutation(np.arange(members.size) % n_fam))}    # every family has a hash
    place = np.sort(rng.choice(n_rec * span, size=n, replace=False))
    occ = np.zeros(n, dtype=SAMPLE_DTYPE)
    occ["iv"], occ["off"] = place // span, place % span
    occ["h0"] = pool[rng.integers(0, pool.size, size=n)]
    return occ, family_of


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_sizes_around_the_sorts_change_of_algorithm(ctx, n):
    occ, family_of = random_occurrences(np.random.default_rng(1700 + n), n, 3, 4, 20 * n)
    got = check(ctx, occ, family_of, 150, 2, f"{n} occurrences")
    assert len(got) > 10 and {s[1] for s in got} == {0, 1, 2}                                  # never a vacuous match


@pytest.fixture(scope="module")
def big():
    "2 * 10^5 occurrences over 40 records and 50 families; (occurrences, family_of, step, min_hits, brute force), made once"
    occ, family_of = random_occurrences(np.random.default_rng(1717), 200_000, 40, 50, 100_000)
    step, min_hits = 2_000, 3
    exp = as_sites(brute_family_sites(zip(occ["h0"].tolist(), occ["iv"].tolist(), occ["off"].tolist()), family_of, step, min_hits))
    return occ, family_of, step, min_hits, exp


def _table(family_of):
    return np.array(sorted(family_of), dtype=np.uint64), np.array([family_of[h] for h in sorted(family_of)], dtype=np.uint32)


def test_random_occurrences(ctx, big):
    occ, family_of, step, min_hits, exp = big
    got = ctx.iv_family_sites(occ, *_table(family_of), step, min_hits)
    print(f"{occ.size} occurrences: {exp.size} sites expected with {int(exp['hits'].sum())} hits, {got.size} returned; "
          f"{np.unique(exp['family']).size} families, {np.unique(exp['rec']).size} records")
    assert exp.size > 5_000 and np.unique(exp["family"]).size == 50 and np.unique(exp["rec"]).size == 40 and int(exp["hits"].max()) > min_hits
    assert got.tobytes() == exp.tobytes()


def test_two_calls_give_the_same_bytes(ctx, big):
    occ, family_of, step, min_hits, _ = big
    hashes, hash_family = _table(family_of)
    assert ctx.iv_family_sites(occ, hashes, hash_family, step, min_hits).tobytes() == ctx.iv_family_sites(occ, hashes, hash_family, step, min_hits).tobytes()


def test_empty_inputs_give_nothing(ctx):
    from ntsynt_amd.device import SAMPLE_DTYPE
    none = np.zeros(0, dtype=SAMPLE_DTYPE)
    assert ctx.iv_family_sites(none, [1, 2], [1, 1], 10, 1).size == 0
    assert ctx.iv_family_sites(occurrences([(1, 0, 0)]), [], [], 10, 1).size == 0
    assert ctx.iv_family_sites(none, [], [], 10, 1).size == 0


def test_errors(ctx):
    from ntsynt_amd.device import NtsError
    a = 0x77
    with pytest.raises(NtsError, match=r"nts_iv_family_sites.*min_hits >= 1.*code -22"):
        ctx.iv_family_sites(occurrences([(a, 0, 0)]), [a], [1], 10, 0)
    with pytest.raises(NtsError, match=r"do not ascend strictly.*code -22"):
        ctx.iv_family_sites(occurrences([(a, 0, 0)]), [5, 5], [1, 1], 10, 1)
    with pytest.raises(NtsError, match=r"do not ascend strictly.*code -22"):
        ctx.iv_family_sites(occurrences([(a, 0, 0)]), [6, 5], [1, 1], 10, 1)
    with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
        occ = occurrences([(a, 0, 0), (a, 1, 1), (a, 2, 2)])
        occ["iv"] = [0, 2, 1]                                                                  # the record decreases
        ctx.iv_family_sites(occ, [a], [1], 10, 1)
    for offs in ([5, 5], [5, 4]):                                                             # the position does not rise
        with pytest.raises(NtsError, match=r"not in \(iv, off\) order.*code -22"):
            occ = occurrences([(a, 0, 0), (a, 0, 1)])
            occ["off"] = offs
            ctx.iv_family_sites(occ, [a], [1], 10, 1)
    with pytest.raises(ValueError, match="one family per hash"):
        ctx.iv_family_sites(occurrences([(a, 0, 0)]), [a], [1, 2], 10, 1)

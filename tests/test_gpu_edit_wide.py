"""The wide pass behind the banded edit distance (csrc/nts_edit_wide.inc, nts_edit_wide) against the full unrestricted table of
tests/wide_brute.py, dist_out and per_iv_out both compared, on hand-made segments of a small uploaded genome pair (the Pair of
tests/test_gpu_edit_segments.py): pure indels of 32 - 1023 bases with and without substitutions beside them, D = E and E + 1 at the
values of E whose rows cross one, two and four lane strides, |dy - dx| = E and E + 1, overband candidates, strings of one base,
flipped pairs of all of these, invalid bases at either end of either string, a segment at base 0 of record 0 and one ending at the
genome's last base, two records, intervals without a segment, what must come back unchanged, 2 000 random segments, n = 0 and an
empty work set (by the timers: no launch), the refused arguments, the same bytes twice.  The cases are built and their expected
results checked on the CPU (case_* functions) before the GPU is called.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B
from tests import wide_brute as W
from tests.test_gpu_edit_segments import Pair, dna, substituted

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
BAND = 31
N_ = np.frombuffer(b"N", dtype=np.uint8)


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ctx():
    from ntsynt_amd.device import Context
    c = Context(0)
    c.profile(True)
    yield c
    c.close()


def add(p, pairs, band=BAND, kinds=None, **kw):
    "an interval whose segments have the kind nts_iv_anchor_segments gives them: offband for |dy - dx| > band, else candidate"
    return p.interval(pairs, kinds=kinds or [B.kind_of(a.size, b.size, band, 65535) for a, b in pairs], **kw)


def inserted(rng, s, at, n, poly=False):
    "n random bases into s at `at` -- or, poly, n times A: a block that offers an alignment nothing but A (a long random one absorbs edits)"
    return np.concatenate([s[:at], np.full(n, ord("A"), np.uint8) if poly else dna(rng, n), s[at:]])


def substituted_not_a(rng, s, places):
    "substituted, each place moved on to the next base that is no A: the edit cannot be made good by a poly-A block"
    return substituted(rng, s, [next(q for q in range(at, s.size) if s[q] != ord("A")) for at in places])


def expected(pair, band, max_edits):
    "(narrow, final, per interval, work set) of the brute force, and the genomes' sequences"
    seqs = []
    for recs in (pair.rec_a, pair.rec_b):
        parts = [np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs]
        seqs.append((np.concatenate(parts), np.concatenate([[0], np.cumsum([x.size for x in parts])[:-1]])))
    (seq_a, off_a), (seq_b, off_b) = seqs
    ivs_a = [(int(off_a[r]) + s, e - s) for r, s, e in pair.iv_a]
    ivs_b = [(int(off_b[r]) + s, e - s) for r, s, e in pair.iv_b]
    return W.brute_wide(seq_a, seq_b, ivs_a, ivs_b, pair.flip, pair.segs, band, max_edits)


def outcomes(pair, exp):
    narrow, final, _, work = exp
    in_work = set(work)
    kinds = [s[5] for s in pair.segs]
    return {"rescued offband": any(kinds[i] == B.OFFBAND and final[i] < B.INVALID for i in work),
            "rescued overband": any(kinds[i] == B.CANDIDATE and final[i] < B.INVALID for i in work),
            "still overband": any(final[i] == B.OVERBAND for i in work),
            "offband overband": any(kinds[i] == B.OFFBAND and final[i] == B.OVERBAND for i in work),
            "invalid in work set": any(final[i] == B.INVALID for i in work),
            "still passed": any(kinds[i] == B.OFFBAND and final[i] == B.PASSED for i in range(len(final))),
            "narrow aligned": any(i not in in_work and narrow[i] < B.INVALID for i in range(len(final))),
            "narrow invalid": any(i not in in_work and narrow[i] == B.INVALID for i in range(len(final))),
            "not candidate": B.NOT_CANDIDATE in final}


def segment_array(pair):
    from ntsynt_amd.device import SEGMENT_DTYPE
    segs = np.array(pair.segs, dtype=np.int64).reshape(-1, 6)
    arr = np.zeros(len(pair.segs), dtype=SEGMENT_DTYPE)
    for c, name in enumerate(SEGMENT_DTYPE.names):
        arr[name] = segs[:, c]
    return arr


def run(ctx, case, what):
    """the two calls against the brute force.  case = (pair, band, E, exp, need): `need` names the outcomes that must occur among the
    expected results -- asserted before the GPU is called"""
    from ntsynt_amd.device import IDENTITY_DTYPE
    pair, band, max_edits, exp, need = case
    narrow, final, exp_iv, work = exp
    seen = outcomes(pair, exp)
    for name in need:
        assert seen[name], (what, "the case has no segment that is", name)
    (ga, _, _), (gb, _, _) = pair.upload(ctx)
    try:
        arr = segment_array(pair)
        _, dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, with_distances=True)
        assert dist.tolist() == narrow, (what, "nts_edit_segments")
        launches = ctx.timing("edit_wide")[1]
        got_iv, got = ctx.edit_wide(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, max_edits, dist)
        launched = ctx.timing("edit_wide")[1] - launches
        again_iv, again = ctx.edit_wide(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, max_edits, dist)
    finally:
        ga.free()
        gb.free()
    bad = [i for i, (g, e) in enumerate(zip(got.tolist(), final)) if g != e][:5]
    print(f"{what}: W {band}, E {max_edits}, {len(pair.segs)} segments in {len(pair.iv_a)} intervals, work set {len(work)}, aligned there "
          f"{sum(final[i] < B.INVALID for i in work)}, overband {sum(final[i] == B.OVERBAND for i in work)}, invalid "
          f"{sum(final[i] == B.INVALID for i in work)}; first differences {bad}")
    assert not bad, (what, [(i, pair.segs[i], got[i], final[i]) for i in bad])
    assert got_iv.dtype == IDENTITY_DTYPE and got_iv.shape == (len(pair.iv_a),)
    for i, e in enumerate(exp_iv):
        assert {n: int(got_iv[i][n]) for n in e} == e, (what, i)
    assert got_iv.tobytes() == again_iv.tobytes() and got.tobytes() == again.tobytes(), what
    assert launched == (1 if work else 0), (what, "launches of k_edit_wide", launched)
    return final


# ---- the cases: built and checked on the CPU

INDELS = (32, 33, 64, 200, 1023)


def case_indels(flip):
    "per length: insertion, deletion, and both with a substitution on either side.  Expected: a pure indel of L bases has D = L"
    rng = np.random.default_rng(10 + flip)
    p = Pair(rng)
    for n in INDELS:
        s = dna(rng, 300)
        ins = inserted(rng, s, 150, n)
        both = substituted_not_a(rng, inserted(rng, s, 150, n, poly=True), [40, 150 + n + 100])
        add(p, [(s, ins)], flip=flip, margin=(3, 5))
        add(p, [(ins, s)], flip=flip, margin=(2, 2))
        add(p, [(s, both)], flip=flip, margin=(0, 4), rec=1)
        add(p, [(both, s)], flip=flip, margin=(4, 0), rec=1)
    exp = expected(p, BAND, 1023)
    final = exp[1]
    for q, n in enumerate(INDELS):
        assert final[4 * q] == n and final[4 * q + 1] == n, (n, final[4 * q:4 * q + 4])
        assert final[4 * q + 2] == final[4 * q + 3] == (n + 2 if n + 2 <= 1023 else B.OVERBAND), (n, final[4 * q:4 * q + 4])
    return p, BAND, 1023, exp, ("rescued offband", "offband overband")


def case_limits(max_edits, flip):
    """D = E and D = E + 1, with delta = 0 (substitutions 20 bases apart; E <= 129), with |delta| = E (a pure indel of E bases, and one
    substitution far from it), and half and half (E >= 127); |delta| = E + 1 stays passed"""
    rng = np.random.default_rng(1000 + 2 * max_edits + flip)
    p = Pair(rng)
    want = []
    if max_edits <= 129:
        s = dna(rng, 20 * (max_edits + 2))
        spaced = lambda m: [10 + 20 * q for q in range(m)]    # noqa: E731
        add(p, [(s, substituted(rng, s, spaced(max_edits)))], flip=flip, margin=(4, 4))
        add(p, [(s, substituted(rng, s, spaced(max_edits + 1)))], flip=flip, margin=(4, 4))
        want += [max_edits, B.OVERBAND]
    s = dna(rng, 600)
    ins = inserted(rng, s, 300, max_edits)
    add(p, [(s, ins)], flip=flip, margin=(1, 1))                                              # |delta| = E = D
    add(p, [(ins, s)], flip=flip, margin=(1, 1), rec=1)
    poly = inserted(rng, s, 300, max_edits, poly=True)
    add(p, [(s, substituted_not_a(rng, poly, [100]))], flip=flip, margin=(1, 1))               # D = E + 1
    add(p, [(substituted_not_a(rng, poly, [500 + max_edits]), s)], flip=flip, margin=(1, 1))
    add(p, [(s, inserted(rng, s, 300, max_edits + 1))], flip=flip, margin=(1, 1))              # |delta| = E + 1: not looked at
    add(p, [(inserted(rng, s, 300, max_edits + 1), s)], flip=flip, margin=(1, 1), rec=1)
    want += [max_edits, max_edits, B.OVERBAND, B.OVERBAND, B.PASSED, B.PASSED]
    if max_edits >= 127:
        half, rest = max_edits // 2, max_edits - max_edits // 2
        s = dna(rng, 4 * rest + 40)
        ins = inserted(rng, s, s.size - 10, half, poly=True)
        at = [5 + 4 * q for q in range(rest + 1)]
        add(p, [(s, substituted(rng, ins, at[:rest]))], flip=flip, margin=(2, 2))            # half an indel, half substitutions: D = E
        add(p, [(s, substituted(rng, ins, at))], flip=flip, margin=(2, 2))                   # D = E + 1
        want += [max_edits, B.OVERBAND]
    exp = expected(p, BAND, max_edits)
    assert exp[1] == want, (max_edits, exp[1], want)
    return p, BAND, max_edits, exp, ("rescued offband", "still overband", "still passed") + (("rescued overband",) if max_edits <= 129 and max_edits > 63 else ())


def case_overband_candidates(flip):
    "delta = 0 with 64 scattered substitutions: D = 64, one more than the narrow pass accepts; beside it what the narrow pass aligns"
    rng = np.random.default_rng(20 + flip)
    p = Pair(rng)
    s = dna(rng, 20 * 70)
    at = [10 + 20 * q for q in range(64)]
    add(p, [(s, substituted(rng, s, at)), (s[:200], substituted(rng, s[:200], [7, 90])), (s, substituted(rng, s, at[:63]))], flip=flip, margin=(5, 5))
    t = dna(rng, 400)
    add(p, [(t, dna(rng, 400))], flip=flip, margin=(0, 0), rec=1)                            # unrelated strings: D far above 63, below 1023
    exp = expected(p, BAND, 1023)
    assert exp[0][:3] == [B.OVERBAND, 2, 63] and exp[1][:3] == [64, 2, 63] and exp[0][3] == B.OVERBAND and 64 < exp[1][3] <= 400, exp[:2]
    return p, BAND, 1023, exp, ("rescued overband", "narrow aligned")


def case_one_base(max_edits, flip):
    "a string of one base against 33 .. E + 1 bases, either way round; one base against one"
    rng = np.random.default_rng(30 + max_edits + flip)
    p = Pair(rng)
    one = dna(rng, 1)
    for n in (33, max_edits, max_edits + 1, max_edits + 2):
        long_b = np.concatenate([dna(rng, n - 1), one]) if n % 2 else np.concatenate([one, dna(rng, n - 1)])
        add(p, [(one, long_b)], flip=flip, margin=(2, 3))
        add(p, [(long_b, one)], flip=flip, margin=(0, 0), rec=1)
    add(p, [(one, one.copy())], flip=flip, margin=(1, 0))
    exp = expected(p, BAND, max_edits)
    assert exp[1] == [32, 32, max_edits - 1, max_edits - 1, max_edits, max_edits, B.PASSED, B.PASSED, 0], exp[1]
    return p, BAND, max_edits, exp, ("rescued offband", "still passed", "narrow aligned")


def case_invalid_bases_edges_records(flip_all):
    """an N at the first and the last base of either string of a work-set segment (offband, and overband candidates), an N in an
    offband segment with |delta| > E (stays passed) and in one with D > E (invalid, not overband); a segment at base 0 of record 0, one
    ending at the genome's last base, two records, intervals without a segment, and what comes back unchanged"""
    rng = np.random.default_rng(40 + flip_all)
    p = Pair(rng)
    s = dna(rng, 400)
    first = add(p, [(s, inserted(rng, s, 200, 50)), (s[:70], s[:70].copy())], flip=False, rec=0)           # base 0 of record 0, no margin
    assert p.iv_a[first][:2] == (0, 0)
    p.filler(0, 37)
    add(p, [], margin=(5, 5))                                                                  # no segment, in the middle of the list
    t = dna(rng, 300)
    wide_b = inserted(rng, t, 150, 60)                                                         # offband, D = 60
    far_b = dna(rng, 300)                                                                      # a candidate far beyond the band, D <= 300
    for flip in ((False, True) if not flip_all else (True, False)):
        for b in (wide_b, far_b):
            add(p, [(np.concatenate([N_, t[1:]]), b)], flip=flip, margin=(2, 2), rec=1)        # invalid first base of A
            add(p, [(np.concatenate([t[:-1], N_]), b)], flip=flip, margin=(2, 2), rec=1)       # invalid last base of A
            add(p, [(t, np.concatenate([N_, b[1:]]))], flip=flip, margin=(2, 2), rec=1)        # of B
            add(p, [(t, np.concatenate([b[:-1], N_]))], flip=flip, margin=(2, 2), rec=1)
            add(p, [(t, b)], flip=flip, margin=(1, 1), rec=1)                                  # the same strings without the N
    n_t = np.concatenate([t[:100], N_, t[101:]])
    add(p, [(n_t, inserted(rng, t, 150, 64))], flip=flip_all, margin=(1, 1))                 # E = 63 below: |delta| = 64 > E, stays passed
    unrelated = inserted(rng, dna(rng, 300), 150, 40)
    add(p, [(n_t, unrelated)], flip=flip_all, margin=(1, 1))                                 # offband, D > 63: invalid goes before overband
    add(p, [(t, unrelated)], flip=flip_all, margin=(1, 1))                                   # the same without the N: overband
    add(p, [(n_t[:150], t[:150].copy())], flip=flip_all, margin=(1, 1))                      # the narrow pass's own invalid
    # kinds that are passed through, beside a work-set segment of the same interval
    add(p, [(t[:30], t[:30].copy()), (t[30:60], t[30:60].copy()), (t[60:], inserted(rng, t[60:], 50, 40)), (t[:9], t[:9].copy())], rec=1,
        kinds=[B.BACKWARD, B.LONG, B.OFFBAND, 7])
    last = add(p, [(s, inserted(rng, substituted(rng, s, [0, 399]), 200, 50))], flip=True, rec=1)          # ends at the genome's last base
    add(p, [], margin=(0, 0))                                                                  # no segment, last in the list (an empty interval)
    p.iv_a[-1] = p.iv_b[-1] = (0, 3, 3)
    assert p.iv_a[last][2] == sum(x.size for x in p.rec_a[1]) and p.iv_b[last][2] == sum(x.size for x in p.rec_b[1])
    exp = expected(p, BAND, 63)
    narrow, final = exp[0], exp[1]
    assert final[0] == 50 and final[1] == 0
    for g in range(4):
        assert final[2 + 5 * g:6 + 5 * g] == [B.INVALID] * 4, (g, final[2 + 5 * g:7 + 5 * g])
    assert [final[6 + 5 * g] for g in range(4)] == [60, B.OVERBAND, 60, B.OVERBAND]
    assert final[22:26] == [B.PASSED, B.INVALID, B.OVERBAND, B.INVALID] and narrow[22:26] == [B.PASSED, B.PASSED, B.PASSED, B.INVALID]
    assert final[26:30] == [B.PASSED, B.PASSED, 40, B.NOT_CANDIDATE] and final[30] == 52
    return p, BAND, 63, exp, ("rescued offband", "still overband", "invalid in work set", "offband overband", "still passed", "narrow aligned", "narrow invalid", "not candidate")


def case_random():
    "2 000 segments of 1 - 300 bases: substitutions 0 - 10 %, a planted indel of 0 - 300 bases in most; a third of the intervals flipped"
    rng = np.random.default_rng(50)
    p = Pair(rng)
    lengths = rng.integers(1, 301, size=2000)
    at = 0
    while at < 2000:
        m = int(rng.integers(1, 21))
        pairs = []
        for n in lengths[at:at + m]:
            a = dna(rng, int(n))
            b = substituted(rng, a, np.flatnonzero(rng.random(a.size) < rng.uniform(0, 0.10)))
            gap = int(rng.integers(0, 301)) if rng.random() < 0.7 else 0
            where = int(rng.integers(0, a.size + 1))
            if rng.random() < 0.5:
                b = inserted(rng, b, where, gap)
            elif a.size - gap >= 1:
                b = np.concatenate([b[:min(where, a.size - gap)], b[min(where, a.size - gap) + gap:]])
            if rng.random() < 0.02:
                b = dna(rng, b.size)
            if rng.random() < 0.01:
                a[rng.integers(0, a.size)] = ord("N")
            pairs.append((a, b))
        add(p, pairs, flip=rng.random() < 1 / 3, rec=int(rng.integers(0, 2)), margin=(int(rng.integers(0, 9)), int(rng.integers(0, 9))))
        at += m
    return p, BAND, 127, expected(p, BAND, 127), ("rescued offband", "rescued overband", "still overband", "offband overband", "invalid in work set",
                                                 "still passed", "narrow aligned", "narrow invalid")


# ---- the tests

@pytest.mark.parametrize("flip", [False, True])
def test_indels_of_32_to_1023_bases(ctx, flip):
    run(ctx, case_indels(flip), f"indels, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("max_edits", [63, 64, 65, 127, 128, 129, 1023])
def test_limits_on_d_and_delta(ctx, max_edits, flip):
    run(ctx, case_limits(max_edits, flip), f"limits at E {max_edits}, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
def test_overband_candidates(ctx, flip):
    run(ctx, case_overband_candidates(flip), f"overband candidates, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("max_edits", [63, 1023])
def test_one_base_against_many(ctx, max_edits, flip):
    run(ctx, case_one_base(max_edits, flip), f"one base, E {max_edits}, flip {flip}")


@pytest.mark.parametrize("flip_all", [False, True])
def test_invalid_bases_edges_records_and_what_stays(ctx, flip_all):
    run(ctx, case_invalid_bases_edges_records(flip_all), f"invalid bases, edges, records; flip {flip_all}")


def test_band_below_31(ctx):
    "W = 7, E = 2 W + 1 = 15, the smallest for that band: an indel of 8 (offband there), of 15 and of 16"
    rng = np.random.default_rng(60)
    p = Pair(rng)
    s = dna(rng, 200)
    add(p, [(s, inserted(rng, s, 100, n)) for n in (8, 15, 16)] + [(s, substituted(rng, s, [5, 50]))], band=7, margin=(3, 3))
    exp = expected(p, 7, 15)
    assert exp[1] == [8, 15, B.PASSED, 2], exp[1]
    run(ctx, (p, 7, 15, exp, ("rescued offband", "still passed", "narrow aligned")), "W 7, E 15")


def test_random_segments(ctx):
    run(ctx, case_random(), "2 000 random segments")


def test_nothing_to_do_launches_nothing(ctx):
    "n = 0, and segments none of which is in the work set: by the timers neither the plan nor the kernel ran"
    rng = np.random.default_rng(70)
    p = Pair(rng)
    add(p, [], margin=(10, 10))
    before = ctx.timing("edit_wide")[1], ctx.timing("edit_wide_plan")[1]
    assert run(ctx, (p, BAND, 1023, expected(p, BAND, 1023), ()), "an interval, no segment") == []
    p = Pair(rng)
    s = dna(rng, 300)
    add(p, [(s, s.copy()), (s, substituted(rng, s, [4, 100])), (s, inserted(rng, s, 100, 1024)), (np.concatenate([N_, s[1:]]), s)], margin=(2, 2))
    exp = expected(p, BAND, 1023)
    assert exp[3] == [] and exp[1] == [0, 2, B.PASSED, B.INVALID]
    run(ctx, (p, BAND, 1023, exp, ("still passed", "narrow aligned", "narrow invalid")), "an empty work set")
    assert (ctx.timing("edit_wide")[1], ctx.timing("edit_wide_plan")[1]) == before


def test_refused_arguments(ctx):
    from ntsynt_amd.device import SEGMENT_DTYPE, NtsError
    rng = np.random.default_rng(80)
    p = Pair(rng)
    s = dna(rng, 50)
    add(p, [(s, s.copy()), (s, inserted(rng, s, 20, 40))], margin=(2, 2))
    add(p, [(s, s.copy())], margin=(2, 2))
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    good = np.array([(0, 2, 50, 2, 50, 0), (0, 52, 50, 52, 90, 3), (1, 2, 50, 2, 50, 0)], dtype=SEGMENT_DTYPE)
    true = np.array([0, B.PASSED, 0], dtype=np.uint32)

    def refused(segs, dist, band=31, max_edits=1023, code="-22"):
        with pytest.raises(NtsError) as err:
            ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, segs, p.flip, band, max_edits, dist)
        assert f"code {code}" in str(err.value), err.value
    try:
        _, dist = ctx.edit_segments(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, with_distances=True)
        assert dist.tolist() == true.tolist()
        per_iv, final = ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, 1023, true)
        assert final.tolist() == [0, 40, 0] and int(per_iv[0]["edits"]) == 40 and int(per_iv[0]["offband"]) == 0
        for band, max_edits in ((0, 1023), (32, 1023), (31, 0), (31, 62), (31, 1024), (7, 14)):
            refused(good, true, band=band, max_edits=max_edits)
        refused(good[::-1].copy(), true[::-1].copy())                                         # not in iv_a order
        # a dist that contradicts its segment's kind
        for at, value in ((0, B.PASSED), (0, B.NOT_CANDIDATE), (0, 64), (1, 5), (1, B.OVERBAND), (1, B.INVALID), (1, B.NOT_CANDIDATE)):
            bad = true.copy()
            bad[at] = value
            refused(good, bad)
        for kind, value in ((B.BACKWARD, 3), (B.LONG, B.NOT_CANDIDATE), (7, B.PASSED)):
            segs, bad = good.copy(), true.copy()
            segs["kind"][2], bad[2] = kind, value
            refused(segs, bad)
        # everything nts_edit_segments refuses of a candidate, and the same of an offband segment of the work set
        for at in (2, 1):
            for field, value in (("iv_a", 2), ("x", 60), ("y_lo", 60), ("dx", 0), ("dy", 0), ("dx", 70000)):
                if at == 1 and field == "iv_a":
                    continue                                  # (that would break the order of the list instead)
                bad = good.copy()
                bad[field][at] = value
                if at == 1 and value == 70000:
                    bad["dy"][at] = 70040                     # (|delta| <= E: still in the work set)
                refused(bad, true)
        outside = good.copy()
        outside["dy"][1] = 2000                               # |delta| > E: not in the work set, not read, not refused
        per_iv, final = ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, outside, p.flip, 31, 1023, true)
        assert final.tolist() == [0, B.PASSED, 0] and int(per_iv[0]["offband"]) == 1
        with pytest.raises(ValueError):
            ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, 1023, true[:2])
        with pytest.raises(ValueError):
            ctx.edit_wide(ga, gb, p.iv_a, p.iv_b[:1], good, p.flip, 31, 1023, true)
    finally:
        ga.free()
        gb.free()

"""The banded edit distance per segment and its sums per interval (csrc/nts_edit.inc, nts_edit_segments) against the full table of
tests/identity_brute.py, dist_out and per_iv_out both compared: hand-made segments on a small uploaded genome pair -- equal strings of
the lengths around the wave and chunk sizes, single edits at the first and last base, indels, |dy - dx| = W, the last accepted and the
first refused value of D + |dy - dx| at W = 31, 7 and 1, flipped pairs, invalid bases at either end of either string, a segment at
base 0 of record 0 and one ending at the genome's last base, two records, intervals without a segment --, 3 000 random segments,
n = 0, the refused arguments, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


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


def dna(rng, n):
    return LETTERS[rng.integers(0, 4, size=n)]


def substituted(rng, s, places):
    out = s.copy()
    for at in places:
        out[at] = rng.choice(LETTERS[LETTERS != out[at]])
    return out


class Pair:
    """two genomes of two records each, grown interval by interval.  An interval holds the strings of its segments one behind the
    other between two margins; B's interval holds the reverse complement of that where the pair is flipped."""

    def __init__(self, rng):
        self.rng = rng
        self.rec_a, self.rec_b = [[], []], [[], []]
        self.iv_a, self.iv_b, self.flip, self.segs = [], [], [], []

    def _at(self, rec):
        return sum(p.size for p in rec)

    def interval(self, pairs, flip=False, rec=0, margin=(0, 0), kinds=None):
        "an interval whose segments are the (A string, B string) pairs; returns its index"
        iv = len(self.iv_a)
        ml, mr = dna(self.rng, margin[0]), dna(self.rng, margin[1])
        a = np.concatenate([ml] + [p[0] for p in pairs] + [mr]) if pairs or margin != (0, 0) else np.zeros(0, np.uint8)
        b = np.concatenate([ml] + [p[1] for p in pairs] + [mr]) if pairs or margin != (0, 0) else np.zeros(0, np.uint8)
        if flip:
            b = B.revcomp(b)
        for seq, recs, ivs in ((a, self.rec_a, self.iv_a), (b, self.rec_b, self.iv_b)):
            at = self._at(recs[rec])
            recs[rec].append(seq)
            ivs.append((rec, at, at + seq.size))
        self.flip.append(1 if flip else 0)
        x, y = margin[0], margin[0]
        for q, (sa, sb) in enumerate(pairs):
            self.segs.append((iv, x, sa.size, y, sb.size, kinds[q] if kinds else B.CANDIDATE))
            x, y = x + sa.size, y + sb.size
        return iv

    def filler(self, rec, n):
        "sequence between intervals, in both genomes"
        self.rec_a[rec].append(dna(self.rng, n))
        self.rec_b[rec].append(dna(self.rng, n))

    def upload(self, ctx):
        from ntsynt_amd.device import Genome
        out = []
        for recs in (self.rec_a, self.rec_b):
            parts = [np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs]
            lens = np.array([p.size for p in parts], dtype=np.uint64)
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            out.append((Genome(ctx, ["r1", "r2"], np.concatenate(parts), offs, lens), np.concatenate(parts), offs))
        return out


def run(ctx, pair, band, what, need=()):
    """the call against the brute force; `need`: outcomes that must occur among the expected results -- asserted before the GPU is
    called"""
    from ntsynt_amd.device import IDENTITY_DTYPE, SEGMENT_DTYPE
    (ga, seq_a, off_a), (gb, seq_b, off_b) = pair.upload(ctx)
    try:
        ivs_a = [(int(off_a[r]) + s, e - s) for r, s, e in pair.iv_a]
        ivs_b = [(int(off_b[r]) + s, e - s) for r, s, e in pair.iv_b]
        exp_dist, exp_iv = B.brute_edit(seq_a, seq_b, ivs_a, ivs_b, pair.flip, pair.segs, band)
        seen = {"aligned": any(d < B.INVALID for d in exp_dist), "overband": B.OVERBAND in exp_dist, "invalid": B.INVALID in exp_dist}
        for name in need:
            assert seen[name], (what, "the case has no segment that is", name)
        segs = np.array(pair.segs, dtype=np.int64).reshape(-1, 6)
        arr = np.zeros(len(pair.segs), dtype=SEGMENT_DTYPE)
        for c, name in enumerate(SEGMENT_DTYPE.names):
            arr[name] = segs[:, c]
        got_iv, got_dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, with_distances=True)
        again_iv, again_dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, with_distances=True)
    finally:
        ga.free()
        gb.free()
    bad = [i for i, (g, e) in enumerate(zip(got_dist.tolist(), exp_dist)) if g != e][:5]
    print(f"{what}: W {band}, {len(pair.segs)} segments in {len(pair.iv_a)} intervals, aligned {sum(d < B.INVALID for d in exp_dist)}, "
          f"overband {exp_dist.count(B.OVERBAND)}, invalid {exp_dist.count(B.INVALID)}; first differences {bad}")
    assert not bad, (what, [(i, pair.segs[i], got_dist[i], exp_dist[i]) for i in bad])
    assert got_iv.dtype == IDENTITY_DTYPE and got_iv.shape == (len(pair.iv_a),)
    for i, e in enumerate(exp_iv):
        assert {n: int(got_iv[i][n]) for n in e} == e, (what, i)
    assert got_iv.tobytes() == again_iv.tobytes() and got_dist.tobytes() == again_dist.tobytes(), what
    return exp_dist


def test_equal_strings_and_single_edits(ctx):
    rng = np.random.default_rng(1)
    p = Pair(rng)
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 4096):
        s = dna(rng, n)
        p.interval([(s, s.copy())], margin=(3, 5))
    s = dna(rng, 200)
    p.interval([(s, substituted(rng, s, [0]))], margin=(2, 2))
    p.interval([(s, substituted(rng, s, [199]))], margin=(2, 2))
    p.interval([(s, np.concatenate([s[:90], dna(rng, 1), s[90:]]))], margin=(1, 1))          # one insertion: dy - dx = 1
    p.interval([(s, np.concatenate([s[:90], s[91:]]))], margin=(1, 1))                       # one deletion: dy - dx = -1
    exp = run(ctx, p, 31, "equal strings, single edits", need=("aligned",))
    assert exp[:9] == [0] * 9 and exp[9:11] == [1, 1] and exp[11] <= 1 and exp[12] <= 1


@pytest.mark.parametrize("band", [31, 7, 1])
def test_band_limits(ctx, band):
    "D + |dy - dx| = 2 W + 1 is the last accepted value, 2 W + 2 the first refused; |dy - dx| = W on both sides; dx = 1 against dy = W + 1"
    rng = np.random.default_rng(100 + band)
    p = Pair(rng)
    s = dna(rng, 40 * (2 * band + 3))
    spaced = lambda m: [20 + 40 * q for q in range(m)]        # noqa: E731 -- substitutions 40 bases apart: each costs exactly one edit
    p.interval([(s, substituted(rng, s, spaced(2 * band + 1)))], margin=(4, 4))
    p.interval([(s, substituted(rng, s, spaced(2 * band + 2)))], margin=(4, 4))
    ins = np.concatenate([s[:310], dna(rng, 1), s[310:]])           # (310: no substitution below falls on the inserted base)
    p.interval([(s, substituted(rng, ins, spaced(2 * band - 1)))], margin=(4, 4))            # D = 2 W, |dy - dx| = 1: 2 W + 1
    p.interval([(s, substituted(rng, ins, spaced(2 * band)))], margin=(4, 4))                # 2 W + 2
    p.interval([(s, np.concatenate([s[:100], dna(rng, band), s[100:]]))], margin=(4, 4))     # dy - dx = W
    p.interval([(s, np.concatenate([s[:100], s[100 + band:]]))], margin=(4, 4))              # dy - dx = -W
    p.interval([(s[:1], np.concatenate([dna(rng, band), s[:1]]))], margin=(4, 4))            # dx = 1, dy = W + 1
    exp = run(ctx, p, band, f"band limits at W {band}", need=("aligned", "overband"))
    assert exp[0] == 2 * band + 1 and exp[1] == B.OVERBAND and exp[2] == 2 * band and exp[3] == B.OVERBAND, exp
    assert exp[4] == band and exp[5] == band and exp[6] == band, exp


def test_flipped_pairs_invalid_bases_edges_and_empty_intervals(ctx):
    rng = np.random.default_rng(2)
    p = Pair(rng)
    s = dna(rng, 500)
    first = p.interval([(s, s.copy()), (s[:70], s[:70].copy())], flip=False, rec=0)          # base 0 of record 0, no margin
    assert p.iv_a[first] == (0, 0, 570)
    p.filler(0, 37)
    p.interval([(s, s.copy())], flip=True, margin=(7, 11))                                   # B is the reverse complement of A: D = 0
    p.interval([(s, substituted(rng, s, [250]))], flip=True, margin=(0, 9))                  # the same with one planted edit
    p.interval([], margin=(5, 5))                                                            # no segment, in the middle of the list
    n = np.frombuffer(b"N", dtype=np.uint8)
    t = dna(rng, 120)
    for flip in (False, True):
        p.interval([(np.concatenate([n, t[1:]]), t.copy())], flip=flip, margin=(2, 2), rec=1)        # invalid first base of A
        p.interval([(np.concatenate([t[:-1], n]), t.copy())], flip=flip, margin=(2, 2), rec=1)       # invalid last base of A
        p.interval([(t.copy(), np.concatenate([n, t[1:]]))], flip=flip, margin=(2, 2), rec=1)        # of B
        p.interval([(t.copy(), np.concatenate([t[:-1], n]))], flip=flip, margin=(2, 2), rec=1)
        p.interval([(t.copy(), t.copy())], flip=flip, margin=(1, 1), rec=1)                          # the same strings without the N: aligned
    # kinds that are passed through, beside a candidate of the same interval
    p.interval([(t[:30], t[:30].copy()), (t[30:60], t[30:60].copy()), (t[60:], t[60:].copy())], rec=1, kinds=[B.BACKWARD, B.CANDIDATE, B.OFFBAND])
    last = p.interval([(s, substituted(rng, s, [0, 499]))], flip=True, rec=1)                # ends at the genome's last base, no margin
    p.interval([], margin=(0, 0))                                                            # no segment, last in the list (an empty interval)
    p.iv_a[-1] = p.iv_b[-1] = (0, 3, 3)
    exp = run(ctx, p, 31, "flips, invalid bases, edges", need=("aligned", "invalid"))
    assert exp[0] == 0 and exp[1] == 0 and exp[2] == 0 and exp[3] == 1
    assert exp[4:9] == [B.INVALID] * 4 + [0] and exp[9:14] == [B.INVALID] * 4 + [0]
    assert exp[14:17] == [B.PASSED, 0, B.PASSED] and exp[17] == 2
    assert p.iv_a[last][2] == sum(x.size for x in p.rec_a[1])


def test_random_segments(ctx):
    "3 000 segments: lengths 1 - 300, a dozen of 2 000 - 4 096; substitutions 0 - 15 %, indels 0 - 3 %; a third of the intervals flipped"
    rng = np.random.default_rng(3)
    p = Pair(rng)
    lengths = rng.integers(1, 301, size=3000)
    lengths[rng.choice(3000, size=12, replace=False)] = rng.integers(2000, 4097, size=12)
    at = 0
    while at < 3000:
        m = int(rng.integers(1, 21))
        pairs = []
        for n in lengths[at:at + m]:
            a = dna(rng, int(n))
            sub, indel = rng.uniform(0, 0.15), rng.uniform(0, 0.03)
            b = substituted(rng, a, np.flatnonzero(rng.random(a.size) < sub))
            out = []
            for c in b:
                r = rng.random()
                if r < indel / 2:
                    continue                                  # a deletion
                out.append(c)
                if r > 1 - indel / 2:
                    out.append(rng.choice(LETTERS))           # an insertion
            b = np.array(out if out else [b[0]], dtype=np.uint8)
            if rng.random() < 0.01:
                a[rng.integers(0, a.size)] = ord("N")
            if abs(int(b.size) - int(a.size)) > 31:           # (what nts_iv_anchor_segments would call offband is no candidate)
                b = a.copy()
            pairs.append((a, b))
        p.interval(pairs, flip=rng.random() < 1 / 3, rec=int(rng.integers(0, 2)), margin=(int(rng.integers(0, 9)), int(rng.integers(0, 9))))
        at += m
    run(ctx, p, 31, "3 000 random segments", need=("aligned", "overband", "invalid"))


def test_nothing_to_do(ctx):
    rng = np.random.default_rng(4)
    p = Pair(rng)
    p.interval([], margin=(10, 10))
    assert run(ctx, p, 31, "an interval, no segment") == []


def test_refused_arguments(ctx):
    from ntsynt_amd.device import SEGMENT_DTYPE, NtsError
    rng = np.random.default_rng(5)
    p = Pair(rng)
    s = dna(rng, 50)
    p.interval([(s, s.copy())], margin=(2, 2))
    p.interval([(s, s.copy())], margin=(2, 2))
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    good = np.array([(0, 2, 50, 2, 50, 0), (1, 2, 50, 2, 50, 0)], dtype=SEGMENT_DTYPE)

    def refused(segs, band=31, code="-22"):
        with pytest.raises(NtsError) as err:
            ctx.edit_segments(ga, gb, p.iv_a, p.iv_b, segs, p.flip, band)
        assert f"code {code}" in str(err.value), err.value
    try:
        ctx.edit_segments(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31)
        refused(good, band=0)
        refused(good, band=32)
        refused(good[::-1].copy())                                                            # not in iv_a order
        for field, value in (("iv_a", 2), ("x", 5), ("y_lo", 5), ("dx", 0), ("dy", 0), ("dy", 90), ("dx", 70000)):
            bad = good.copy()
            bad[field][1] = value
            refused(bad)
        with pytest.raises(ValueError):
            ctx.edit_segments(ga, gb, p.iv_a, p.iv_b[:1], good, p.flip, 31)
    finally:
        ga.free()
        gb.free()

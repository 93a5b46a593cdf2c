"""The edit script per segment (csrc/nts_edit_script.inc, nts_edit_script) against the full table and the walk of
tests/variants_brute.py, op by op, and separately: the ops applied to A give B.  Hand-made segments on a small uploaded genome pair of
two records (the Pair of tests/test_gpu_edit_segments.py): only equal strings, single edits at the first and last base, the
homopolymer and the SUB-versus-indel ties, the lengths around the ballot's 64 positions, |dy - dx| = W, the largest accepted D + |dy -
dx|, flipped pairs of all of these, the genome's first and last base, segments that are not aligned between aligned ones, 2 000
random segments, n = 0, a dist that is not the segments' own, the same bytes twice.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B
from tests import variants_brute as V
from tests.test_gpu_edit_segments import LETTERS, Pair, dna, substituted

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


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


def s(text):
    return np.frombuffer(text.encode(), dtype=np.uint8).copy()


def segment_array(pair):
    from ntsynt_amd.device import SEGMENT_DTYPE
    segs = np.array(pair.segs, dtype=np.int64).reshape(-1, 6)
    arr = np.zeros(len(pair.segs), dtype=SEGMENT_DTYPE)
    for c, name in enumerate(SEGMENT_DTYPE.names):
        arr[name] = segs[:, c]
    return arr


def expected(pair, seq_a, off_a, seq_b, off_b, band):
    "(dist, ops as tuples, first, the two strings of every aligned segment) from the brute forces"
    ivs_a = [(int(off_a[r]) + x, e - x) for r, x, e in pair.iv_a]
    ivs_b = [(int(off_b[r]) + x, e - x) for r, x, e in pair.iv_b]
    dist, _ = B.brute_edit(seq_a, seq_b, ivs_a, ivs_b, pair.flip, pair.segs, band)
    ops, first, strings = [], [0], {}
    for i, (seg, d) in enumerate(zip(pair.segs, dist)):
        if d < B.INVALID:
            a, b = B.strings_of(seq_a, seq_b, ivs_a[seg[0]], ivs_b[seg[0]], pair.flip[seg[0]], seg)
            strings[i] = (a, b)
            mine = V.op_records(i, a, b)
            assert len(mine) == d
            ops += mine
        first.append(len(ops))
    return dist, ops, first, strings


def run(ctx, pair, band, what, need_ops=True):
    "the call against the brute force; returns (expected dist, expected ops)"
    from ntsynt_amd.device import OP_DTYPE
    (ga, seq_a, off_a), (gb, seq_b, off_b) = pair.upload(ctx)
    try:
        dist, ops, first, strings = expected(pair, seq_a, off_a, seq_b, off_b, band)
        assert bool(ops) == need_ops, (what, "the case has no op" if need_ops else "the case has ops")
        arr = segment_array(pair)
        _, got_dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, with_distances=True)
        assert got_dist.tolist() == dist, what
        got, got_first = ctx.edit_script(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, got_dist)
        again, again_first = ctx.edit_script(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, got_dist)
    finally:
        ga.free()
        gb.free()
    assert got.dtype == OP_DTYPE and got_first.dtype == np.uint64
    assert got_first.tolist() == first, what
    rows = [tuple(r)[:6] for r in got.tolist()]
    bad = [i for i, (g, e) in enumerate(zip(rows, ops)) if g != e][:5]
    print(f"{what}: W {band}, {len(pair.segs)} segments, {sum(d < B.INVALID for d in dist)} aligned, {sum(1 <= d < B.INVALID for d in dist)} with D >= 1, "
          f"{len(ops)} ops; first differences {bad}")
    assert len(rows) == len(ops) and not bad, (what, [(rows[i], ops[i]) for i in bad])
    assert not got["pad"].any()
    # separately: the ops applied to A give B
    for i, (a, b) in strings.items():
        mine = got[int(got_first[i]):int(got_first[i + 1])]
        assert (mine["seg"] == i).all()
        as_brute = [(int(o["op"]), int(o["p"]), int(o["q"]), None if o["base_b"] == 0xFF else int(ASCII[o["base_b"]])) for o in mine]
        assert V.apply_script(a, as_brute).tobytes() == b.tobytes(), (what, i)
    assert got.tobytes() == again.tobytes() and got_first.tobytes() == again_first.tobytes(), what
    return dist, ops


def spaced(m, step=40):
    return [20 + step * q for q in range(m)]


def hand_cases(rng, band):
    "(name, A, B) of every hand-made case that fits the band"
    t = dna(rng, 200)
    out = [("SUB at the first base", t, substituted(rng, t, [0])), ("SUB at the last base", t, substituted(rng, t, [199])),
           ("DEL of the first base", t, t[1:]), ("DEL of the last base", t, t[:-1]),
           ("INS before the first base", t, np.concatenate([dna(rng, 1), t])), ("INS behind the last base", t, np.concatenate([t, dna(rng, 1)])),
           ("homopolymer run that lost a base", s("GAAAC"), s("GAAC")), ("homopolymer at the string's start", s("AAAC"), s("AAC")),
           ("homopolymer run that gained a base", s("GAAC"), s("GAAAC")), ("two SUBs, not DEL + INS", s("AC"), s("CA")),
           ("two SUBs inside", s("GGACTT"), s("GGCATT"))]
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 4096):
        u = dna(rng, n)
        out.append((f"length {n}, one edit in the middle", u, substituted(rng, u, [n // 2])))
    for n in (64, 65, 128, 129):                              # the mismatch exactly 64 and 128 positions back from the corner, and one more
        u = dna(rng, n + 1)
        out.append((f"length {n + 1}, the edit {n} positions back", u, substituted(rng, u, [0])))
    u = dna(rng, 300)
    out.append((f"dy - dx = {band}", u, np.concatenate([u[:100], dna(rng, band), u[100:]])))
    out.append((f"dy - dx = -{band}", u, np.concatenate([u[:100], u[100 + band:]])))
    out.append((f"dx = 1, dy = {band + 1}", u[:1], np.concatenate([dna(rng, band), u[:1]])))
    out.append((f"dx = {band + 1}, dy = 1", np.concatenate([dna(rng, band), u[:1]]), u[:1]))
    return out


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("band", [31, 7, 1])
def test_hand_cases(ctx, band, flip):
    rng = np.random.default_rng(10 + band)
    p = Pair(rng)
    names = []
    for name, a, b in hand_cases(rng, band):
        p.interval([(a, b)], flip=flip, margin=(3, 5), rec=len(names) % 2)
        names.append(name)
    dist, ops = run(ctx, p, band, f"hand cases, W {band}, flip {flip}")
    of = dict(zip(names, dist))
    assert all(of[n] == 1 for n in names if "first base" in n or "last base" in n or "one edit" in n or "positions back" in n or "homopolymer" in n), of
    assert of["two SUBs, not DEL + INS"] == 2 and of[f"dy - dx = {band}"] == band and of[f"dy - dx = -{band}"] == band
    by_seg = {}
    for o in ops:
        by_seg.setdefault(names[o[0]], []).append(o[1:4])
    assert by_seg["homopolymer run that lost a base"] == [(1, 1, V.DEL)] and by_seg["homopolymer at the string's start"] == [(0, 0, V.DEL)]
    assert by_seg["homopolymer run that gained a base"] == [(1, 1, V.INS)]
    assert by_seg["two SUBs, not DEL + INS"] == [(0, 0, V.SUB), (1, 1, V.SUB)]
    assert by_seg["INS before the first base"] == [(0, 0, V.INS)]


@pytest.mark.parametrize("flip", [False, True])
def test_the_largest_accepted_distance(ctx, flip):
    """W = 31: D + |dy - dx| = 62 and 63 -- 63 is the last value nts_edit_segments returns as a distance, (D + |dy - dx|) // 2 = 31 --
    at dy - dx = 0, 31 and -31: up to 64 rows of F"""
    band = 31
    rng = np.random.default_rng(31)
    p = Pair(rng)
    t = dna(rng, 40 * 66)
    want = []
    for total in (62, 63):
        p.interval([(t, substituted(rng, t, spaced(total)))], flip=flip, margin=(4, 4))
        want.append(total)
        ins = np.concatenate([t[:310], dna(rng, band), t[310:]])    # (310: no substitution below falls on an inserted base)
        p.interval([(t, substituted(rng, ins, spaced(total - 2 * band)))], flip=flip, margin=(4, 4))
        want.append(total - band)
        p.interval([(substituted(rng, ins, spaced(total - 2 * band)), t)], flip=flip, margin=(4, 4))
        want.append(total - band)
    dist, _ = run(ctx, p, band, f"largest accepted distances, flip {flip}")
    assert dist == want, dist


def test_edges_of_the_genome_and_segments_that_are_not_aligned(ctx):
    rng = np.random.default_rng(2)
    p = Pair(rng)
    t = dna(rng, 500)
    first = p.interval([(t, substituted(rng, t, [0, 250])), (t[:70], substituted(rng, t[:70], [69]))], flip=False, rec=0)   # base 0 of record 0
    assert p.iv_a[first] == (0, 0, 570)
    p.filler(0, 37)
    n = np.frombuffer(b"N", dtype=np.uint8)
    u = dna(rng, 120)
    far = substituted(rng, u, list(range(0, 120, 2)))         # 60 substitutions at W = 7: overband
    for flip in (False, True):
        p.interval([(u[:30], substituted(rng, u[:30], [3])), (u[30:60], u[30:60].copy()), (u[60:], substituted(rng, u[60:], [0]))], flip=flip, rec=1,
                   kinds=[B.BACKWARD, B.CANDIDATE, B.OFFBAND])
        p.interval([(u, substituted(rng, u, [7])), (np.concatenate([n, u[1:]]), u.copy()), (u, substituted(rng, u, [5, 100])), (u, far),
                    (u, np.concatenate([u[:50], u[53:]])), (u[:40], u[:40].copy()), (u, substituted(rng, u, [119]))], flip=flip, rec=1, margin=(2, 2),
                   kinds=[B.CANDIDATE, B.CANDIDATE, B.CANDIDATE, B.CANDIDATE, B.CANDIDATE, B.LONG, B.CANDIDATE])
        p.interval([], margin=(5, 5), rec=1)                  # an interval without a segment
    last = p.interval([(t, substituted(rng, t, [0, 499]))], flip=True, rec=1)                # ends at the genome's last base
    dist, ops = run(ctx, p, 7, "edges, passed and refused segments between aligned ones")
    assert p.iv_a[last][2] == sum(x.size for x in p.rec_a[1])
    assert dist[:2] == [2, 1] and dist[-1] == 2
    for at in (2, 12):
        assert dist[at:at + 10] == [B.PASSED, 0, B.PASSED, 1, B.INVALID, 2, B.OVERBAND, 3, B.PASSED, 1], dist
    assert {o[0] for o in ops} == {0, 1, 5, 7, 9, 11, 15, 17, 19, 21, 22}


def test_only_equal_strings(ctx):
    rng = np.random.default_rng(3)
    p = Pair(rng)
    for n in (1, 64, 300):
        u = dna(rng, n)
        p.interval([(u, u.copy()), (u, u.copy())], flip=n == 64, margin=(1, 1))
    dist, ops = run(ctx, p, 31, "only D = 0", need_ops=False)
    assert dist == [0] * 6 and ops == []


def test_nothing_to_do(ctx):
    rng = np.random.default_rng(4)
    p = Pair(rng)
    p.interval([], margin=(10, 10))
    dist, ops = run(ctx, p, 31, "an interval, no segment", need_ops=False)
    assert dist == [] and ops == []


def test_random_segments(ctx):
    "2 000 segments of 1 - 300 bases with 0 - 6 planted edits; a third of the intervals flipped"
    rng = np.random.default_rng(5)
    p = Pair(rng)
    at = 0
    while at < 2000:
        m = min(int(rng.integers(1, 21)), 2000 - at)
        pairs = []
        for _ in range(m):
            a = dna(rng, int(rng.integers(1, 301)))
            b = list(a)
            for _ in range(int(rng.integers(0, 7)) if rng.random() < 0.6 else 0):
                kind, where = int(rng.integers(0, 3)), int(rng.integers(0, len(b)))
                if kind == 0:
                    b[where] = rng.choice(LETTERS[LETTERS != b[where]])
                elif kind == 1 and len(b) > 1:
                    del b[where]
                else:
                    b.insert(where, rng.choice(LETTERS))
            pairs.append((a, np.array(b, dtype=np.uint8)))
        p.interval(pairs, flip=rng.random() < 1 / 3, rec=int(rng.integers(0, 2)), margin=(int(rng.integers(0, 9)), int(rng.integers(0, 9))))
        at += m
    (seq_a, off_a), (seq_b, off_b) = host_sequences(p)
    dist, ops, _, _ = expected(p, seq_a, off_a, seq_b, off_b, 31)
    assert len(dist) == 2000 and sum(1 <= d < B.INVALID for d in dist) * 3 >= 2000, "fewer than a third of the segments have an edit"
    assert {o[3] for o in ops} == {V.SUB, V.DEL, V.INS}
    run(ctx, p, 31, "2 000 random segments")


def host_sequences(pair):
    "(concatenated records, record offsets) of the two genomes, as Pair.upload lays them out"
    out = []
    for recs in (pair.rec_a, pair.rec_b):
        parts = [np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs]
        lens = np.array([x.size for x in parts], dtype=np.uint64)
        out.append((np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)))
    return out


def test_refused_arguments_and_a_dist_that_is_not_the_segments_own(ctx):
    from ntsynt_amd.device import SEGMENT_DTYPE, NtsError
    rng = np.random.default_rng(6)
    p = Pair(rng)
    t = dna(rng, 50)
    p.interval([(t, substituted(rng, t, [10, 30]))], margin=(2, 2))
    p.interval([(t, t.copy())], margin=(2, 2))
    p.interval([(t, np.concatenate([t[:20], t[23:]]))], margin=(2, 2))
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    good = segment_array(p)
    true = np.array([2, 0, 3], dtype=np.uint32)

    def refused(segs, dist, band=31, code="-22", says=None):
        with pytest.raises(NtsError) as err:
            ctx.edit_script(ga, gb, p.iv_a, p.iv_b, segs, p.flip, band, dist)
        assert f"code {code}" in str(err.value), err.value
        assert says is None or says in str(err.value), err.value
    try:
        ops, first = ctx.edit_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, true)
        assert first.tolist() == [0, 2, 2, 5] and ops["seg"].tolist() == [0, 0, 2, 2, 2]
        # a dist one too small and one too large on one segment: found by the kernel, nothing returned
        refused(good, np.array([1, 0, 3], dtype=np.uint32), says="dist is not the distance of segment 0")
        refused(good, np.array([2, 0, 4], dtype=np.uint32), says="dist is not the distance of segment 2")
        refused(good, np.array([2, 1, 3], dtype=np.uint32), says="dist is not the distance of segment 1")
        # refused before any launch: a distance beyond the band (here |dy - dx| = 3 at W = 7: at most 2 * 7 + 1 - 3), one on a segment
        # that is no candidate, and everything nts_edit_segments refuses
        refused(good, np.array([2, 0, 13], dtype=np.uint32), band=7, says="beyond the band")
        refused(good, np.array([16, 0, 3], dtype=np.uint32), band=7, says="beyond the band")
        passed = good.copy()
        passed["kind"][1] = B.LONG
        refused(passed, true, says="no candidate")
        ops, first = ctx.edit_script(ga, gb, p.iv_a, p.iv_b, passed, p.flip, 31, np.array([2, B.PASSED, 3], dtype=np.uint32))
        assert first.tolist() == [0, 2, 2, 5] and ops.size == 5
        refused(good, true, band=0)
        refused(good, true, band=32)
        refused(good[::-1].copy(), true)
        for field, value in (("iv_a", 3), ("x", 5), ("y_lo", 9), ("dx", 0), ("dy", 0), ("dy", 90), ("dx", 70000)):
            bad = good.copy()
            bad[field][2] = value
            refused(bad, true)
        with pytest.raises(ValueError):
            ctx.edit_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, true[:2])
        with pytest.raises(ValueError):
            ctx.edit_script(ga, gb, p.iv_a, p.iv_b[:1], good, p.flip, 31, true)
        empty = np.zeros(0, dtype=SEGMENT_DTYPE)
        ops, first = ctx.edit_script(ga, gb, p.iv_a, p.iv_b, empty, p.flip, 31, np.zeros(0, dtype=np.uint32))
        assert ops.size == 0 and first.tolist() == [0]
        # the context still works after the refusals
        ops, first = ctx.edit_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, true)
        assert first.tolist() == [0, 2, 2, 5]
    finally:
        ga.free()
        gb.free()

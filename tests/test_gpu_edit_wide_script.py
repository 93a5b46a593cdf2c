"""The edit scripts of the stretches beyond the band (csrc/nts_edit_wide_script.inc, nts_edit_wide_script) against the full table and
walk of tests/variants_brute.py, on hand-made segments of the small two-record Pair of tests/test_gpu_edit_segments.py: ops and `first`
compared entry by entry, the ops applied to A give B, every case in `+` and flipped.  Pure indels of 32 - 1023 bases, the same inside a
homopolymer and after a base equal to the indel's first base, delta = 0 with 64 - 1023 substitutions, D = E, one base against many,
SUB, DEL and INS in one script, match runs around the ballot's 64 positions, the genome's first and last base, what is no member
between members, the same bytes at the default and at the smallest budget and on a second call, n = 0 and an empty script set (no
launch, by the timers), the refused arguments, a dist that is off by one.  The cases are built and their expected results checked on
the CPU before the GPU is called.  Every test runs under a time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B
from tests import variants_brute as V
from tests import wide_brute as W
from tests import wide_variants_brute as WV
from tests.test_gpu_edit_segments import Pair, dna, substituted
from tests.test_gpu_edit_wide import add, inserted, segment_array, substituted_not_a

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
BAND = 31
ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)
N_ = np.frombuffer(b"N", dtype=np.uint8)
POLY = lambda n, c="A": np.full(n, ord(c), np.uint8)          # noqa: E731


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


def min_budget(max_edits):
    return 4 * (max_edits + 1) ** 2


def expected(pair, band, max_edits):
    "(narrow, final, ops, first, members, the two strings of every member) of the brute forces"
    seqs = []
    for recs in (pair.rec_a, pair.rec_b):
        parts = [np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs]
        seqs.append((np.concatenate(parts), np.concatenate([[0], np.cumsum([x.size for x in parts])[:-1]])))
    (seq_a, off_a), (seq_b, off_b) = seqs
    ivs_a = [(int(off_a[r]) + s, e - s) for r, s, e in pair.iv_a]
    ivs_b = [(int(off_b[r]) + s, e - s) for r, s, e in pair.iv_b]
    narrow, final, _, _ = W.brute_wide(seq_a, seq_b, ivs_a, ivs_b, pair.flip, pair.segs, band, max_edits)
    ops, first, members = WV.expected_ops(seq_a, seq_b, ivs_a, ivs_b, pair.flip, pair.segs, final, band)
    strings = {i: B.strings_of(seq_a, seq_b, ivs_a[pair.segs[i][0]], ivs_b[pair.segs[i][0]], pair.flip[pair.segs[i][0]], pair.segs[i]) for i in members}
    return narrow, final, ops, first, members, strings


def run(ctx, pair, band, max_edits, exp, what, budgets=(0,)):
    "the calls against the brute force; exp = expected(...), checked by the case before the GPU is called.  Returns the ops' bytes"
    from ntsynt_amd.device import OP_DTYPE
    narrow, final, ops, first, members, strings = exp
    (ga, _, _), (gb, _, _) = pair.upload(ctx)
    try:
        arr = segment_array(pair)
        _, dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, with_distances=True)
        assert dist.tolist() == narrow, (what, "nts_edit_segments")
        _, got_final = ctx.edit_wide(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, max_edits, dist)
        assert got_final.tolist() == final, (what, "nts_edit_wide")
        launches = ctx.timing("edit_wide_script")[1]
        results, plans = [], []
        for budget in tuple(budgets) + (budgets[0],):         # (the first budget twice: the same bytes on a second call)
            results.append(ctx.edit_wide_script(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, band, max_edits, got_final, table_budget=budget))
            plans.append(ctx.edit_wide_script_last_plan())
        launched = ctx.timing("edit_wide_script")[1] - launches
    finally:
        ga.free()
        gb.free()
    got, got_first = results[0]
    assert got.dtype == OP_DTYPE and got_first.dtype == np.uint64
    assert got_first.tolist() == first, what
    rows = [tuple(r)[:6] for r in got.tolist()]
    bad = [i for i, (g, e) in enumerate(zip(rows, ops)) if g != e][:5]
    print(f"{what}: W {band}, E {max_edits}, {len(pair.segs)} segments, {len(members)} members, {len(ops)} ops, plans {plans}; first differences {bad}")
    assert len(rows) == len(ops) and not bad, (what, [(rows[i], ops[i]) for i in bad])
    assert not got["pad"].any()
    for i, (a, b) in strings.items():                         # separately: the ops applied to A give B
        mine = got[int(got_first[i]):int(got_first[i + 1])]
        assert mine.size == final[i] and (mine["seg"] == i).all()
        as_brute = [(int(o["op"]), int(o["p"]), int(o["q"]), None if o["base_b"] == 0xFF else int(ASCII[o["base_b"]])) for o in mine]
        assert V.apply_script(a, as_brute).tobytes() == b.tobytes(), (what, i)
    for other, other_first in results[1:]:
        assert other.tobytes() == got.tobytes() and other_first.tobytes() == got_first.tobytes(), what
    assert launched == (len(results) if members else 0), (what, "timed launches", launched)
    for plan in plans:
        assert plan["members"] == len(members) and plan["table_bytes"] == sum(4 * (final[i] + 1) ** 2 for i in members), (what, plan)
    return got.tobytes(), plans


def kinds_of_ops(exp, i):
    return {op[3] for op in exp[2][exp[3][i]:exp[3][i + 1]]}


# ---- the cases: built and checked on the CPU

INDELS = (32, 63, 64, 65, 300, 1023)


def case_pure_indels(flip):
    "insertion and deletion per length: D = |delta|, every pruned row is one diagonal wide, the script is one run of INS or of DEL"
    rng = np.random.default_rng(100 + flip)
    p = Pair(rng)
    for n in INDELS:
        s = dna(rng, 240)
        ins = inserted(rng, s, 120, n)
        add(p, [(s, ins)], flip=flip, margin=(3, 5))
        add(p, [(ins, s)], flip=flip, margin=(2, 2), rec=1)
    exp = expected(p, BAND, 1023)
    assert exp[1] == [n for n in INDELS for _ in (0, 1)] and exp[4] == list(range(2 * len(INDELS)))
    for q in range(len(INDELS)):
        assert kinds_of_ops(exp, 2 * q) == {V.INS} and kinds_of_ops(exp, 2 * q + 1) == {V.DEL}
    return p, BAND, 1023, exp


def case_indel_ties(flip):
    """the same indels inside a homopolymer (rule 1 matches back through the run: the indel comes out at the run's first base) and after
    a base equal to the indel's first base (the indel moves one base to the left or splits)"""
    rng = np.random.default_rng(110 + flip)
    p = Pair(rng)
    for n in INDELS:
        left, right = dna(rng, 120), dna(rng, 120)
        left[-1], right[0] = ord("C"), ord("G")
        run_a, run_b = np.concatenate([left, POLY(20), right]), np.concatenate([left, POLY(20 + n), right])
        add(p, [(run_a, run_b)], flip=flip, margin=(2, 3))
        add(p, [(run_b, run_a)], flip=flip, margin=(2, 3), rec=1)
        s = dna(rng, 240)
        block = dna(rng, n)
        block[0], block[-1] = s[119], s[119]                  # the indel repeats the base in front of it, first and last
        tie = np.concatenate([s[:120], block, s[120:]])
        add(p, [(s, tie)], flip=flip, margin=(1, 1))
        add(p, [(tie, s)], flip=flip, margin=(1, 1), rec=1)
    exp = expected(p, BAND, 1023)
    assert exp[1] == [n for n in INDELS for _ in range(4)]
    ops, first = exp[2], exp[3]
    for q in range(len(INDELS)):                              # the homopolymer: the run's first bases are the ones inserted / deleted
        assert ops[first[4 * q]][1:3] == (120, 120) and ops[first[4 * q + 1]][1:3] == (120, 120), ops[first[4 * q]]
    return p, BAND, 1023, exp


def case_substitutions(flip):
    "delta = 0 with D = 64, 65, 128, 129 and 1023 spaced substitutions: overband candidates; the row strides change at 64 and 128"
    rng = np.random.default_rng(120 + flip)
    p = Pair(rng)
    want = []
    for d, step in ((64, 10), (65, 10), (128, 8), (129, 8), (1023, 4)):
        s = dna(rng, step * d + 40)
        add(p, [(s, substituted(rng, s, [20 + step * q for q in range(d)]))], flip=flip, margin=(4, 4), rec=d % 2)
        want.append(d)
    exp = expected(p, BAND, 1023)
    assert exp[0] == [B.OVERBAND] * 5 and exp[1] == want and exp[4] == list(range(5)), exp[1]
    assert all(kinds_of_ops(exp, i) == {V.SUB} for i in range(5))
    return p, BAND, 1023, exp


def case_d_equals_e(max_edits, flip):
    """D = E: a pure indel of E bases either way round, E spaced substitutions (delta = 0), half and half; D = E + 1 beside them is no
    member, and at E = 63 = 2 W + 1 the substitutions are nts_edit_script's (D + |delta| <= 2 W + 1): no member either"""
    rng = np.random.default_rng(1300 + 2 * max_edits + flip)
    p = Pair(rng)
    s = dna(rng, 300)
    ins = inserted(rng, s, 150, max_edits)
    add(p, [(s, ins)], flip=flip, margin=(1, 1))
    add(p, [(ins, s)], flip=flip, margin=(1, 1), rec=1)
    poly = inserted(rng, s, 150, max_edits, poly=True)
    add(p, [(s, substituted_not_a(rng, poly, [60]))], flip=flip, margin=(1, 1))             # D = E + 1: overband, no member
    step = 10 if max_edits <= 128 else 4
    t = dna(rng, step * max_edits + 40)
    at = [20 + step * q for q in range(max_edits + 1)]
    add(p, [(t, substituted(rng, t, at[:max_edits]))], flip=flip, margin=(2, 2), rec=1)
    half, rest = max_edits // 2, max_edits - max_edits // 2
    u = dna(rng, 4 * rest + 40)
    mixed = inserted(rng, u, u.size - 10, half, poly=True)
    add(p, [(u, substituted(rng, mixed, [5 + 4 * q for q in range(rest)]))], flip=flip, margin=(2, 2))
    exp = expected(p, BAND, max_edits)
    assert exp[1] == [max_edits, max_edits, B.OVERBAND, max_edits, max_edits], (max_edits, exp[1])
    assert exp[4] == ([0, 1, 3, 4] if max_edits > 2 * BAND + 1 else [0, 1, 4]) and exp[3][2] == exp[3][3]
    return p, BAND, max_edits, exp


def case_one_base(max_edits, flip):
    "one base against 33, E and E + 1 bases, either way round"
    rng = np.random.default_rng(140 + max_edits + flip)
    p = Pair(rng)
    one = dna(rng, 1)
    for n in (33, max_edits, max_edits + 1):
        long_b = np.concatenate([dna(rng, n - 1), one]) if n % 2 else np.concatenate([one, dna(rng, n - 1)])
        add(p, [(one, long_b)], flip=flip, margin=(2, 3))
        add(p, [(long_b, one)], flip=flip, margin=(0, 0), rec=1)
    exp = expected(p, BAND, max_edits)
    assert exp[1] == [32, 32, max_edits - 1, max_edits - 1, max_edits, max_edits], exp[1]
    return p, BAND, max_edits, exp


def case_mixed_and_runs(flip):
    """an indel of 40 and 30 substitutions (SUB, DEL and INS in one script); match runs of 63, 64, 65 and 200 bases between the corner
    and the last mismatch, and between two mismatches"""
    rng = np.random.default_rng(150 + flip)
    p = Pair(rng)
    s = dna(rng, 700)
    b = inserted(rng, substituted(rng, s, [10 + 20 * q for q in range(15)]), 330, 40)        # 15 SUBs, 40 INS,
    b = substituted(rng, b, [400 + 20 * q for q in range(15)])                              # 15 SUBs,
    a = inserted(rng, s, 650, 36)                                                            # and 36 DEL
    add(p, [(a, b)], flip=flip, margin=(3, 3))
    for run in (63, 64, 65, 200):
        t = dna(rng, 500)
        u = inserted(rng, substituted(rng, t, [499 - run, 499 - run - 1 - run]), 50, 45)     # run matches, a mismatch, run matches, a mismatch
        add(p, [(t, u)], flip=flip, margin=(2, 2), rec=1)
        add(p, [(u, t)], flip=flip, margin=(2, 2))
    exp = expected(p, BAND, 1023)
    assert kinds_of_ops(exp, 0) == {V.SUB, V.DEL, V.INS} and exp[1][0] <= 106, exp[1][0]
    assert exp[1][1:] == [47] * 8 and exp[4] == list(range(9))
    return p, BAND, 1023, exp


def case_edges_and_non_members(flip_all):
    """a member at base 0 of record 0 and one ending at the genome's last base; between members what must add nothing to `first`:
    narrow-aligned, invalid (narrow and wide), overband, passed (|delta| > E), backward, long and other kinds, an interval without a
    segment"""
    rng = np.random.default_rng(160 + flip_all)
    p = Pair(rng)
    s = dna(rng, 300)
    first = add(p, [(s, inserted(rng, s, 150, 50)), (s[:70], s[:70].copy())], flip=False, rec=0)           # base 0 of record 0, no margin
    assert p.iv_a[first][:2] == (0, 0)
    p.filler(0, 37)
    add(p, [], margin=(5, 5))
    t = dna(rng, 200)
    n_t = np.concatenate([t[:100], N_, t[101:]])
    add(p, [(t, substituted(rng, t, [5, 90])),                                                # narrow-aligned, D = 2
            (t, inserted(rng, t, 100, 60)),                                                   # member, D = 60
            (n_t, t.copy()),                                                                   # the narrow pass's invalid
            (n_t, inserted(rng, t, 100, 40)),                                                  # the wide pass's invalid
            (t, inserted(rng, t, 100, 64)),                                                    # E = 63 below: |delta| > E, stays passed
            (t, inserted(rng, dna(rng, 200), 100, 40)),                                        # offband, D > E: overband
            (t, t.copy()),                                                                     # D = 0
            (inserted(rng, t, 30, 33), t)], flip=flip_all, margin=(2, 2), rec=1)               # member, D = 33
    add(p, [(t[:30], t[:30].copy()), (t[30:60], t[30:60].copy()), (t[60:], inserted(rng, t[60:], 50, 40)), (t[:9], t[:9].copy())], rec=1,
        kinds=[B.BACKWARD, B.LONG, B.OFFBAND, 7], flip=flip_all)
    last = add(p, [(s, inserted(rng, substituted(rng, s, [0, 299]), 150, 50))], flip=True, rec=1)          # ends at the genome's last base
    assert p.iv_a[last][2] == sum(x.size for x in p.rec_a[1]) and p.iv_b[last][2] == sum(x.size for x in p.rec_b[1])
    exp = expected(p, BAND, 63)
    assert exp[1] == [50, 0, 2, 60, B.INVALID, B.INVALID, B.PASSED, B.OVERBAND, 0, 33, B.PASSED, B.PASSED, 40, B.NOT_CANDIDATE, 52], exp[1]
    assert exp[4] == [0, 3, 9, 12, 14]
    return p, BAND, 63, exp


def case_random_members(max_edits, extra=()):
    "500 members with an indel of 32 - 200 bases and a few substitutions, a third of the intervals flipped; `extra`: larger indels behind them"
    rng = np.random.default_rng(170 + max_edits)
    p = Pair(rng)
    sizes = [int(x) for x in rng.integers(32, 201, size=500)] + list(extra)
    at = 0
    while at < len(sizes):
        m = int(rng.integers(1, 21))
        pairs = []
        for gap in sizes[at:at + m]:
            a = dna(rng, int(rng.integers(60, 200)))
            b = substituted(rng, a, np.flatnonzero(rng.random(a.size) < 0.02))
            b = inserted(rng, b, int(rng.integers(0, a.size + 1)), gap)
            pairs.append((a, b) if rng.random() < 0.5 else (b, a))
        add(p, pairs, flip=rng.random() < 1 / 3, rec=int(rng.integers(0, 2)), margin=(int(rng.integers(0, 9)), int(rng.integers(0, 9))))
        at += m
    exp = expected(p, BAND, max_edits)
    assert len(exp[4]) == len(sizes), (len(exp[4]), "members")
    return p, BAND, max_edits, exp


# ---- the tests

@pytest.mark.parametrize("flip", [False, True])
def test_pure_indels_of_32_to_1023_bases(ctx, flip):
    p, band, e, exp = case_pure_indels(flip)
    run(ctx, p, band, e, exp, f"pure indels, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
def test_indels_in_a_homopolymer_and_after_an_equal_base(ctx, flip):
    p, band, e, exp = case_indel_ties(flip)
    run(ctx, p, band, e, exp, f"indel ties, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
def test_delta_0_with_64_to_1023_substitutions(ctx, flip):
    p, band, e, exp = case_substitutions(flip)
    run(ctx, p, band, e, exp, f"substitutions, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("max_edits", [63, 64, 127, 128, 1023])
def test_d_equals_e(ctx, max_edits, flip):
    p, band, e, exp = case_d_equals_e(max_edits, flip)
    run(ctx, p, band, e, exp, f"D = E = {max_edits}, flip {flip}", budgets=(0, min_budget(max_edits)))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("max_edits", [63, 1023])
def test_one_base_against_many(ctx, max_edits, flip):
    p, band, e, exp = case_one_base(max_edits, flip)
    run(ctx, p, band, e, exp, f"one base, E {max_edits}, flip {flip}")


@pytest.mark.parametrize("flip", [False, True])
def test_sub_del_ins_in_one_script_and_match_runs_around_64(ctx, flip):
    p, band, e, exp = case_mixed_and_runs(flip)
    run(ctx, p, band, e, exp, f"mixed script and match runs, flip {flip}")


@pytest.mark.parametrize("flip_all", [False, True])
def test_genome_edges_and_what_is_no_member(ctx, flip_all):
    p, band, e, exp = case_edges_and_non_members(flip_all)
    run(ctx, p, band, e, exp, f"edges and non-members, flip {flip_all}", budgets=(0, min_budget(e)))


def test_the_budget_does_not_change_a_byte(ctx):
    "500 random members: the default budget in one batch, the smallest in many; at E = 1023 members of D = 1023 are a batch each"
    p, band, e, exp = case_random_members(255)
    _, plans = run(ctx, p, band, e, exp, "500 random members, E 255", budgets=(0, min_budget(255)))
    assert plans[0]["batches"] == 1 and plans[1]["batches"] >= 100, plans
    p, band, e, exp = case_random_members(1023, extra=(1023, 1023, 1000, 1023))
    _, plans = run(ctx, p, band, e, exp, "500 random members and four large ones, E 1023", budgets=(0, min_budget(1023)))
    final, members = exp[1], exp[4]
    alone = sum(final[i] == 1023 for i in members)
    assert alone >= 3 and plans[0]["batches"] == 1 and plans[1]["batches"] >= alone + 2, (plans, alone)


def test_nothing_to_do_launches_nothing(ctx):
    "n = 0 and an empty script set: by the timers neither the plan nor the kernel ran; (no ops, first all 0)"
    rng = np.random.default_rng(180)
    before = ctx.timing("edit_wide_script")[1], ctx.timing("edit_wide_script_plan")[1]
    p = Pair(rng)
    add(p, [], margin=(10, 10))
    exp = expected(p, BAND, 1023)
    assert exp[2] == [] and exp[3] == [0]
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    try:
        ops, first = ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, segment_array(p), p.flip, BAND, 1023, np.zeros(0, np.uint32))
    finally:
        ga.free()
        gb.free()
    assert ops.size == 0 and first.tolist() == [0]
    p = Pair(rng)
    s = dna(rng, 300)
    add(p, [(s, s.copy()), (s, substituted(rng, s, [4, 100])), (s, inserted(rng, s, 100, 1024)), (np.concatenate([N_, s[1:]]), s)], margin=(2, 2))
    exp = expected(p, BAND, 1023)
    assert exp[1] == [0, 2, B.PASSED, B.INVALID] and exp[4] == [] and exp[3] == [0] * 5
    got, plans = run(ctx, p, BAND, 1023, exp, "an empty script set")
    assert got == b"" and plans[0] == {"members": 0, "table_bytes": 0, "batches": 0}
    assert (ctx.timing("edit_wide_script")[1], ctx.timing("edit_wide_script_plan")[1]) == before


def test_refused_arguments_and_a_dist_off_by_one(ctx):
    from ntsynt_amd.device import NtsError
    rng = np.random.default_rng(190)
    p = Pair(rng)
    s = dna(rng, 50)
    add(p, [(s, s.copy()), (s, inserted(rng, s, 20, 40))], margin=(2, 2))
    add(p, [(s, substituted_not_a(rng, inserted(rng, s, 30, 35, poly=True), [3])), (s, substituted(rng, s, [7]))], margin=(2, 2))
    exp = expected(p, BAND, 1023)
    assert exp[1] == [0, 40, 36, 1] and exp[4] == [1, 2] and exp[3] == [0, 0, 40, 76, 76]
    good, true = segment_array(p), np.array(exp[1], dtype=np.uint32)
    assert good["kind"].tolist() == [B.CANDIDATE, B.OFFBAND, B.OFFBAND, B.CANDIDATE]
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    timers = lambda: (ctx.timing("edit_wide_script")[1], ctx.timing("edit_wide_script_plan")[1])      # noqa: E731

    def refused(segs, dist, band=31, max_edits=1023, budget=0, code="-22", words="", launched=False):
        before = timers()
        with pytest.raises(NtsError) as err:
            ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, segs, p.flip, band, max_edits, dist, table_budget=budget)
        assert f"code {code}" in str(err.value) and words in str(err.value), err.value
        assert (timers() != before) == launched, (words, "refused before any launch" if not launched else "refused after the launch")
    try:
        ops, first = ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, 1023, true)
        assert first.tolist() == exp[3] and ops.size == 76
        for band, max_edits in ((0, 1023), (32, 1023), (31, 0), (31, 62), (31, 1024), (7, 14)):
            refused(good, true, band=band, max_edits=max_edits)
        refused(good, true, budget=min_budget(1023) - 1, words="table_budget")
        refused(good, true, budget=1, words="table_budget")
        refused(good, true, max_edits=63, budget=min_budget(63) - 1, words="table_budget")
        assert ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, 63, true, table_budget=min_budget(63))[0].tobytes() == ops.tobytes()
        refused(good[::-1].copy(), true[::-1].copy())                                           # not in iv_a order
        for kind in (B.BACKWARD, B.LONG, 7):                                                    # a distance on a kind that has none
            segs = good.copy()
            segs["kind"][3] = kind
            refused(segs, true, words="neither candidate nor offband")
        over = true.copy()
        over[1] = 64
        refused(good, over, max_edits=63, words="beyond max_edits")                             # D > E
        below = true.copy()
        below[1] = 39
        refused(good, below, words="below the difference")                                      # D < |delta|
        level, zero = good.copy(), true.copy()
        level["dy"][1], zero[1] = 50, 0                                                         # offband by its kind, but dx = dy and D = 0:
        refused(level, zero, words="a distance of 0 on segment 1")                              # every member has D >= 1
        # everything nts_edit_segments refuses of a candidate, and the same of an offband member
        for at in (3, 1):
            for field, value in (("x", 60), ("y_lo", 100), ("dx", 0), ("dx", 70000)):
                bad = good.copy()
                bad[field][at] = value
                if at == 1 and field == "dx":
                    bad["dy"][at] = value + 40                # (|delta| stays 40 = D)
                refused(bad, true)
        with pytest.raises(ValueError):
            ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, good, p.flip, 31, 1023, true[:2])
        with pytest.raises(ValueError):
            ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b[:1], good, p.flip, 31, 1023, true)
        # a member's D changed by one either way: refused after the launch, naming that segment, no ops
        for at, step in ((1, 1), (2, 1), (2, -1)):
            off = true.copy()
            off[at] = int(off[at]) + step
            refused(good, off, words=f"dist is not the distance of segment {at}", launched=True)
        off = true.copy()
        off[1], off[2] = 41, 35
        refused(good, off, words="dist is not the distance of segment 1", launched=True)       # the smallest such index
    finally:
        ga.free()
        gb.free()


def test_2_to_the_32_edits_are_refused_before_any_launch(ctx):
    """NTS_ERANGE for a sum of D of 2^32 or more, decided on the host: 4 198 405 copies of one offband segment of 1 base against 1 024
    with D = 1 023, the least number that reaches the bound (the segments may overlap).  By the timers nothing was launched; three of
    the same segments are accepted."""
    from ntsynt_amd.device import NtsError
    rng = np.random.default_rng(200)
    p = Pair(rng)
    one = dna(rng, 1)
    add(p, [(one, np.concatenate([dna(rng, 1023), one]))])
    assert p.segs == [(0, 0, 1, 0, 1024, B.OFFBAND)]
    copies = -(-2 ** 32 // 1023)
    assert copies == 4_198_405 and (copies - 1) * 1023 < 2 ** 32 <= copies * 1023
    segs = np.repeat(segment_array(p), copies)
    dist = np.full(copies, 1023, dtype=np.uint32)
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    timers = lambda: (ctx.timing("edit_wide_script")[1], ctx.timing("edit_wide_script_plan")[1])      # noqa: E731
    try:
        before = timers()
        with pytest.raises(NtsError) as err:
            ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, segs, p.flip, BAND, 1023, dist)
        assert "code -34" in str(err.value) and "2^32 edits" in str(err.value), err.value
        assert timers() == before, "refused before any launch"
        assert ctx.edit_wide_script_last_plan() == {"members": 0, "table_bytes": 0, "batches": 0}
        ops, first = ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, segs[:3], p.flip, BAND, 1023, dist[:3])   # the same segments, few of them
        assert first.tolist() == [0, 1023, 2046, 3069] and ops.size == 3069 and (ops["op"] == 3).all()
    finally:
        ga.free()
        gb.free()

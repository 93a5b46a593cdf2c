"""The edit script of an extended flank (csrc/nts_edit_extend_script.inc, nts_edit_extend_script) against the definition: the expected
ops are tests/variants_brute.script on A' and B' as tests/extend_brute.task_strings reads them, cut to the (ext_a, ext_b) that
tests/extend_brute.extend_brute gives -- the `results` handed to the GPU come from that brute force, not from the GPU.  A small
uploaded genome pair of two records each (the World of tests/test_gpu_edit_extend.py).  D = 0 only (by the timer: no launch), D = 1,
no bases; D = 31 .. 129 (the rows where lanes stride once, twice and four times); D = 255 and D = 1023; match runs of 0 .. 129 bases
between two edits and in front of the first; scripts that begin with a deletion or an insertion of 1, 5 and 40 bases; indels of 1 ..
40 bases with a substitution directly beside them; indels inside a homopolymer and a dinucleotide repeat; all eight flag combinations
(eight equal op lists); record limits and seams; invalid bases directly behind ext_a and ext_b; 2 000 random tasks; a chained case
whose results come from ctx.edit_extend; the budget (one batch per member, the same ops, one byte less refused); every refusal; the
same bytes twice.  Every case is built and its expected values asserted on the CPU before the GPU is called.  Every test runs under a
time limit of its own."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import extend_brute as X
from tests import variants_brute as V
from tests.test_gpu_edit_extend import LETTERS, N_, World, dna, substituted, task_array, unlike

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
SUB, DEL, INS = V.SUB, V.DEL, V.INS


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


def letters(text):
    return np.frombuffer(text.encode(), dtype=np.uint8).copy()


def result_array(results):
    from ntsynt_amd.device import EXTEND_DTYPE
    arr = np.zeros(len(results), dtype=EXTEND_DTYPE)
    for q, r in enumerate(results):
        arr[q] = tuple(r)
    return arr


def expected(world, penalty, max_edits):
    """per task: (the brute force's five fields, the op records of the canonical script of A' and B', A', B'); the script has `edits`
    ops and turns A' into B'"""
    ra, rb = world.records()
    out = []
    for q, t in enumerate(world.tasks):
        a, b = X.task_strings(ra, rb, t)
        res, _ = X.extend_brute(a, b, penalty, max_edits)
        a1, b1 = a[:res[0]], b[:res[1]]
        ops = V.op_records(q, a1, b1)
        assert len(ops) == res[2], (q, len(ops), res)
        rebuilt = V.apply_script(a1, [(op, p, qq, int(b1[qq]) if op != DEL else None) for _, p, qq, op, _, _ in ops])
        assert np.array_equal(rebuilt, b1), q
        out.append((res, ops, a1, b1))
    return out


def compare(got_ops, got_first, exp, what):
    from ntsynt_amd.device import OP_DTYPE
    want = [op + (0,) for e in exp for op in e[1]]
    first = np.concatenate([[0], np.cumsum([len(e[1]) for e in exp])]).astype(np.uint64)
    assert got_ops.dtype == OP_DTYPE and got_ops.shape == (len(want),), (what, got_ops.shape, len(want))
    assert np.array_equal(got_first, first), what
    got = [tuple(o) for o in got_ops.tolist()]
    bad = [q for q, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    print(f"{what}: {len(exp)} tasks, {len(want)} ops, largest D {max([len(e[1]) for e in exp], default=0)}; first differences {bad}")
    assert not bad, (what, [(q, got[q], want[q]) for q in bad])


def run(ctx, case, what, budget=0):
    "case = (world, expected): the call, twice, against the expected ops; returns the ops"
    world, exp = case
    ga, gb = world.upload(ctx)
    try:
        arr, res = task_array(world.tasks), result_array([e[0] for e in exp])
        launches = ctx.timing("edit_extend_script")[1]
        ops, first = ctx.edit_extend_script(ga, gb, arr, res, budget)
        launched = ctx.timing("edit_extend_script")[1] - launches
        plan = ctx.edit_extend_script_last_plan()
        again, first_again = ctx.edit_extend_script(ga, gb, arr, res, budget)
    finally:
        ga.free()
        gb.free()
    compare(ops, first, exp, what)
    assert ops.tobytes() == again.tobytes() and first.tobytes() == first_again.tobytes(), what
    members = [len(e[1]) for e in exp if e[1]]
    assert launched == (1 if members else 0), (what, "timed groups of k_edit_extend_script", launched)
    assert plan["members"] == len(members) and plan["table_bytes"] == sum(4 * (d + 1) ** 2 for d in members), (what, plan)
    return ops, plan


# ---- the cases: built and checked on the CPU

def case_no_edit():
    "identical strings, strings of no base: every D is 0"
    rng = np.random.default_rng(101)
    w = World(rng)
    s = dna(rng, 300)
    none = np.zeros(0, np.uint8)
    for a, b, flags in ((s, s.copy(), 0), (s[:64], s[:65], 3), (none, s, 0), (s, none, 7), (none, none, 0)):
        w.place(a, b, flags=flags, rec=flags & 1)
    exp = expected(w, 6, 255)
    assert all(e[0][2] == 0 and not e[1] for e in exp), exp
    return w, exp


def case_small():
    "D = 1 of each kind, ext_a = ext_b = 0 between them"
    rng = np.random.default_rng(102)
    w = World(rng)
    s = dna(rng, 200)
    w.place(s, substituted(rng, s, [80]))
    w.place(letters("A" * 30), letters("C" * 30), rec=1)       # (nothing aligns: ext_a = ext_b = 0)
    w.place(s, np.delete(s, 90), flags=3, rec=1)
    w.place(np.delete(s, 70), s, flags=6)
    exp = expected(w, 6, 255)
    assert [e[0][2] for e in exp] == [1, 0, 1, 1] and exp[1][0][:2] == (0, 0), [e[0] for e in exp]
    assert [e[1][0][3] for e in exp if e[1]] == [SUB, DEL, INS], exp
    return w, exp


ROWS = (31, 32, 33, 63, 64, 65, 127, 128, 129)


def case_rows():
    "substitutions 20 bases apart up to the strings' common end: scripts of exactly 31 .. 129 ops"
    rng = np.random.default_rng(103)
    w = World(rng)
    for q, edits in enumerate(ROWS):
        s = dna(rng, 20 * edits + 15)
        w.place(s, substituted(rng, s, [10 + 20 * x for x in range(edits)]), flags=(0, 3, 6, 5)[q % 4], rec=q % 2)
    exp = expected(w, 6, 255)
    assert [e[0][2] for e in exp] == list(ROWS), [e[0] for e in exp]
    return w, exp


def case_many_edits(edits):
    "penalty 3, a substitution at every fourth base up to the common end: the brute force's winner spends all `edits`"
    rng = np.random.default_rng(500 + edits)
    w = World(rng)
    s = dna(rng, 4 * edits + 3)
    w.place(s, substituted(rng, s, [3 + 4 * x for x in range(edits)]), flags=3 if edits > 255 else 0)
    exp = expected(w, 3, edits)
    assert exp[0][0][:3] == (s.size, s.size, edits), exp[0][0]
    return w, exp


RUNS = (0, 1, 63, 64, 65, 128, 129)


def case_match_runs():
    """a run of r matching bases, a substitution, a run of r' matching bases, a substitution, 90 matching bases -- r and r' over 0 .. 129
    -- and a deletion of A's first base in front of a run of 63 .. 129 bases that is all of B' (the walk reaches j = 0 by matches),
    an insertion likewise (i = 0)"""
    rng = np.random.default_rng(104)
    w = World(rng)
    want = []
    for q, front in enumerate(RUNS):
        for between in RUNS:
            s = dna(rng, front + between + 92)
            places = [front, front + 1 + between]
            w.place(s, substituted(rng, s, places), flags=(0, 3, 6)[q % 3], rec=q % 2)
            want.append([(SUB, p, p) for p in places])
    for front in RUNS[2:]:
        s = dna(rng, front)
        extra = unlike(rng, s[:1])                             # (one base in front that the other string lacks)
        w.place(np.concatenate([extra, s]), s.copy())
        want.append([(DEL, 0, 0)])
        w.place(s.copy(), np.concatenate([extra, s]), flags=3, rec=1)
        want.append([(INS, 0, 0)])
    exp = expected(w, 3, 255)
    got = [[(op, p, q) for _, p, q, op, _, _ in e[1]] for e in exp]
    assert got == want, [(q, g, x) for q, (g, x) in enumerate(zip(got, want)) if g != x][:5]
    return w, exp


def case_leading_indels():
    "scripts that begin with a deletion or an insertion of 1, 5 and 40 bases: the walk ends along column 0 or row 0"
    rng = np.random.default_rng(105)
    w = World(rng)
    want = []
    for n in (1, 5, 40):
        s = dna(rng, 300)
        extra = np.concatenate([dna(rng, n - 1), unlike(rng, s[:1])]) if n > 1 else unlike(rng, s[:1])
        extra[0] = unlike(rng, s[:1])[0] if n > 1 and extra[0] == s[0] else extra[0]
        w.place(np.concatenate([extra, s]), s.copy(), flags=0)
        want.append((DEL, n))
        w.place(s.copy(), np.concatenate([extra, s]), flags=7, rec=1)
        want.append((INS, n))
    exp = expected(w, 3, 255)
    for (kind, n), e in zip(want, exp):
        ops = [(op, p, q) for _, p, q, op, _, _ in e[1]]
        assert e[0][2] >= n and ops[0] == (kind, 0, 0) and [o[0] for o in ops[:n]] == [kind] * n, (kind, n, e[0], ops[:3])
    return w, exp


def case_indels_beside_substitutions():
    """one insertion or deletion of 1 .. 40 bases 150 bases in, with a substitution directly in front of it or directly behind it; the
    inserted bases are none of the two beside them, so that no script of fewer edits absorbs the substitution"""
    rng = np.random.default_rng(106)
    w = World(rng)
    want = []
    for n in range(1, 41):
        s = dna(rng, 400)
        free = LETTERS[(LETTERS != s[149]) & (LETTERS != s[150])]
        ins = np.concatenate([s[:150], free[rng.integers(0, free.size, size=n)], s[150:]])
        for at in (149, 150 + n):
            both = substituted(rng, ins, [at])
            w.place(s, both, rec=n % 2, flags=(0, 3)[n % 2])
            w.place(both, s, rec=n % 2, flags=(6, 5)[n % 2])
            want += [(n + 1, INS), (n + 1, DEL)]
    exp = expected(w, 3, 255)
    for (edits, kind), e in zip(want, exp):
        kinds = [o[3] for o in e[1]]
        assert e[0][2] == edits and min(e[0][:2]) == 400 and kinds.count(kind) == edits - 1 and kinds.count(SUB) == 1, (edits, kind, e[0])
    return w, exp


def case_repeats():
    """two bases fewer or more in a run of ten A, one unit fewer or more in (AC) x 8: the canonical walk takes matches first from the
    end, so the indel lies at the repeat's first bases in the strings as read"""
    rng = np.random.default_rng(107)
    w = World(rng)
    left, right = np.concatenate([dna(rng, 99), letters("G")]), np.concatenate([letters("T"), dna(rng, 149)])

    def around(middle):
        return np.concatenate([left, letters(middle), right])
    pairs = [("A" * 10, "A" * 8, DEL, 2), ("A" * 8, "A" * 10, INS, 2), ("AC" * 8, "AC" * 7, DEL, 2), ("AC" * 7, "AC" * 8, INS, 2)]
    for a, b, _, _ in pairs:
        for flags in (0, 3):
            w.place(around(a), around(b), flags=flags, rec=flags & 1)
    exp = expected(w, 3, 255)
    for q, e in enumerate(exp):
        _, _, kind, n = pairs[q // 2]
        ops = [(op, p, qq) for _, p, qq, op, _, _ in e[1]]
        assert e[0][2] == n and ops == [(kind, 100 + x if kind == DEL else 100, 100 if kind == DEL else 100 + x) for x in range(n)], (q, e[0], ops)
    return w, exp


def case_directions():
    "one pair of strings under all eight combinations of the three flags: eight op lists equal but for seg"
    rng = np.random.default_rng(108)
    w = World(rng)
    s = dna(rng, 260)
    a = np.concatenate([s, dna(rng, 40)])
    b = np.concatenate([substituted(rng, np.concatenate([s[:90], dna(rng, 7), s[90:140], s[143:]]), [30, 200]), dna(rng, 40)])
    for flags in range(8):
        w.filler(flags & 1, 5)
        w.place(a, b, flags=flags, rec=flags & 1)
    exp = expected(w, 6, 255)
    assert all(e[0] == exp[0][0] and [o[1:] for o in e[1]] == [o[1:] for o in exp[0][1]] for e in exp) and exp[0][0][2] >= 12, exp[0][0]
    assert {o[3] for o in exp[0][1]} == {SUB, DEL, INS}
    return w, exp


def case_record_limits():
    """a backwards string that ends at base 0 of record 0, a forwards one that ends at the last base of the last record, strings that
    touch the seam between the records from both sides -- in either genome"""
    rng = np.random.default_rng(109)
    w = World(rng)
    s = dna(rng, 120)
    t = np.delete(substituted(rng, s, [70, 118]), 30)
    first = w.place(s, t, flags=3, rec=0)
    w.filler(0, 9)
    seam_left = w.place(s, t, flags=0, rec=0)
    seam_right = w.place(s, t, flags=3, rec=1)
    w.filler(1, 9)
    last = w.place(s, t, flags=0, rec=1)
    ra, rb = w.records()
    assert w.tasks[first][1] == 119 and w.tasks[first][4] == 118 and w.tasks[seam_right][1] == 119
    assert w.tasks[seam_left][1] + 120 == ra[0].size and w.tasks[seam_left][4] + 119 == rb[0].size
    assert w.tasks[last][1] + 120 == ra[1].size and w.tasks[last][4] + 119 == rb[1].size
    w.tasks.append((0, w.tasks[seam_left][1], 120, 1, w.tasks[seam_right][4], 119, 2))
    w.tasks.append((1, 119, 120, 0, w.tasks[seam_left][4], 119, 1))
    exp = expected(w, 3, 255)
    assert all(e[0] == (120, 119, 3, 120, 119) for e in exp), [e[0] for e in exp]
    return w, exp


def case_invalid_behind():
    "an N directly behind ext_a, directly behind ext_b, behind both: the strings are cut there and the script ends in front of it"
    rng = np.random.default_rng(110)
    w = World(rng)
    s = dna(rng, 200)
    t = substituted(rng, s, [50, 120])
    tail = dna(rng, 30)
    for flags in (0, 7):
        w.place(np.concatenate([s, N_, tail]), np.concatenate([t, tail, tail]), flags=flags)
        w.place(np.concatenate([s, tail, tail]), np.concatenate([t, N_, tail]), flags=flags, rec=1)
        w.place(np.concatenate([s, N_, tail]), np.concatenate([t, N_, tail]), flags=flags)
    exp = expected(w, 6, 255)
    assert all(e[0][:3] == (200, 200, 2) and (e[0][3] == 200 or e[0][4] == 200) for e in exp), [e[0] for e in exp]
    return w, exp


def case_random(seed, tasks):
    "strings of 50 .. 400 bases, 0 .. 8 % substitutions, now and then an indel of 1 .. 12 bases, mixed flags: P = 6, E = 255"
    rng = np.random.default_rng(seed)
    w = World(rng)
    for _ in range(tasks):
        s = dna(rng, int(rng.integers(50, 401)))
        b = substituted(rng, s, np.flatnonzero(rng.random(s.size) < rng.uniform(0.0, 0.08)))
        while rng.random() < 0.35:
            at, n = int(rng.integers(0, b.size)), int(rng.integers(1, 13))
            b = np.concatenate([b[:at], dna(rng, n), b[at:]]) if rng.random() < 0.5 else np.delete(b, slice(at, at + n))
        if b.size == 0:
            b = s[:1].copy()
        flags = int(rng.integers(0, 8))
        w.place(s, b, flags=flags, rec=int(rng.integers(0, 2)))
    exp = expected(w, 6, 255)
    kinds = [o[3] for e in exp for o in e[1]]
    assert sum(not e[1] for e in exp) >= tasks // 100 and kinds.count(DEL) >= tasks // 10 and kinds.count(INS) >= tasks // 10
    assert max(e[0][2] for e in exp) >= 30
    return w, exp


# ---- the tests

def test_no_edit_launches_nothing(ctx):
    before = ctx.timing("edit_extend_script")[1], ctx.timing("edit_extend_script_plan")[1]
    ops, plan = run(ctx, case_no_edit(), "D = 0 only")
    assert ops.size == 0 and plan == {"members": 0, "table_bytes": 0, "batches": 0}
    assert (ctx.timing("edit_extend_script")[1], ctx.timing("edit_extend_script_plan")[1]) == before
    rng = np.random.default_rng(100)
    w = World(rng)
    w.filler(0, 10)
    w.filler(1, 10)
    run(ctx, (w, []), "no task")
    assert (ctx.timing("edit_extend_script")[1], ctx.timing("edit_extend_script_plan")[1]) == before


def test_one_edit_and_no_bases(ctx):
    run(ctx, case_small(), "D = 1")


def test_rows_where_the_lane_strides_change(ctx):
    run(ctx, case_rows(), "D = 31 .. 129")


@pytest.mark.parametrize("edits", [255, 1023])
def test_many_edits(ctx, edits):
    _, plan = run(ctx, case_many_edits(edits), f"D = {edits}")
    assert plan["table_bytes"] == 4 * (edits + 1) ** 2 and plan["batches"] == 1


def test_match_runs_around_the_ballot(ctx):
    run(ctx, case_match_runs(), "match runs")


def test_scripts_that_begin_with_an_indel(ctx):
    run(ctx, case_leading_indels(), "leading indels")


def test_indels_with_a_substitution_beside_them(ctx):
    run(ctx, case_indels_beside_substitutions(), "indels beside substitutions")


def test_indels_inside_repeats(ctx):
    run(ctx, case_repeats(), "repeats")


def test_all_eight_directions(ctx):
    ops, _ = run(ctx, case_directions(), "directions")
    per_task = ops.reshape(8, -1)
    for q in range(8):
        assert (per_task[q]["seg"] == q).all()
        for field in ("p", "q", "op", "base_a", "base_b", "pad"):
            assert np.array_equal(per_task[q][field], per_task[0][field]), (q, field)


def test_record_limits_and_seams(ctx):
    run(ctx, case_record_limits(), "record limits")


def test_invalid_bases_directly_behind_the_extension(ctx):
    run(ctx, case_invalid_behind(), "invalid bases behind the extension")


def test_two_thousand_random_tasks(ctx):
    run(ctx, case_random(120, 2000), "2 000 random tasks")


def test_results_of_the_extension_kernel(ctx):
    "chained: the results come from ctx.edit_extend (which the brute force confirms), the ops from them"
    world, exp = case_random(121, 200)
    ga, gb = world.upload(ctx)
    try:
        arr = task_array(world.tasks)
        results = ctx.edit_extend(ga, gb, arr, 6, 255)
        ops, first = ctx.edit_extend_script(ga, gb, arr, results)
    finally:
        ga.free()
        gb.free()
    assert [tuple(r) for r in results.tolist()] == [e[0] for e in exp]
    compare(ops, first, exp, "chained")


def test_budget_cuts_batches_and_changes_nothing(ctx):
    "seven members of D = 5 between tasks of D = 0: at 4 x 36 bytes every member is its own batch"
    from ntsynt_amd.device import NtsError
    rng = np.random.default_rng(122)
    w = World(rng)
    for q in range(10):
        s = dna(rng, 150)
        w.place(s, s.copy() if q in (0, 4, 9) else substituted(rng, s, [20, 40, 60, 80, 100]), flags=q % 8, rec=q % 2)
    exp = expected(w, 6, 255)
    assert [e[0][2] for e in exp] == [0 if q in (0, 4, 9) else 5 for q in range(10)]
    whole, plan = run(ctx, (w, exp), "budget 0")
    assert plan == {"members": 7, "table_bytes": 7 * 144, "batches": 1}
    cut, plan = run(ctx, (w, exp), "budget 144", budget=144)
    assert plan == {"members": 7, "table_bytes": 7 * 144, "batches": 7}
    assert cut.tobytes() == whole.tobytes()
    two, plan = run(ctx, (w, exp), "budget 300", budget=300)
    assert plan["batches"] == 4 and two.tobytes() == whole.tobytes()
    ga, gb = w.upload(ctx)
    try:
        before = ctx.timing("edit_extend_script")[1]
        with pytest.raises(NtsError) as err:
            ctx.edit_extend_script(ga, gb, task_array(w.tasks), result_array([e[0] for e in exp]), 143)
        assert "code -22" in str(err.value) and "table_budget" in str(err.value), err.value
        assert ctx.timing("edit_extend_script")[1] == before
    finally:
        ga.free()
        gb.free()


def refusal_world():
    rng = np.random.default_rng(123)
    w = World(rng)
    s = dna(rng, 100)
    for q in range(6):
        w.place(s, substituted(rng, s, [20, 50, 80]), flags=(0, 3)[q % 2], rec=q % 2)
    w.filler(0, 5)
    exp = expected(w, 6, 255)
    assert all(e[0] == (100, 100, 3, 100, 100) for e in exp)
    return w, exp


def test_refusals_before_the_launch_write_nothing(ctx):
    from ntsynt_amd.device import EXTEND_DTYPE
    w, exp = refusal_world()
    good_tasks = [tuple(t) for t in w.tasks]
    good_results = [e[0] for e in exp]
    ga, gb = w.upload(ctx)

    def refused(tasks, results, names, budget=0):
        tk, rs = task_array(tasks), result_array(results)
        assert rs.dtype == EXTEND_DTYPE
        p, m = ctypes.c_void_p(0x5A5A5A5A), ctypes.c_uint64(0xA5A5A5A5)
        first = np.full(len(tasks) + 1, 0xABABABABABABABAB, dtype=np.uint64)
        before = ctx.timing("edit_extend_script")[1], ctx.timing("edit_extend_script_plan")[1]
        rc = ctx.lib.nts_edit_extend_script(ctx.h, ga.h, gb.h, tk.ctypes.data, tk.size, rs.ctypes.data, budget, ctypes.byref(p), ctypes.byref(m),
                                            first.ctypes.data)
        message = ctx.lib.nts_last_error(ctx.h).decode()
        assert rc == -22, (rc, message)
        assert names in message, (names, message)
        assert p.value == 0x5A5A5A5A and m.value == 0xA5A5A5A5 and (first == 0xABABABABABABABAB).all(), "a refused call wrote to its outputs"
        assert (ctx.timing("edit_extend_script")[1], ctx.timing("edit_extend_script_plan")[1]) == before
    try:
        for at, field, value in ((2, 2, 65536), (2, 5, 65536), (3, 6, 8), (3, 6, 1 << 31), (2, 0, 2), (2, 3, 2),
                                 (2, 2, 400), (3, 1, 98), (3, 4, 98), (3, 1, 5000)):
            for also in (None, 5):                             # (a second offending task behind it: the smallest is named)
                bad = [list(t) for t in good_tasks]
                bad[at][field] = value
                if also is not None:
                    bad[also][6] = 8
                refused([tuple(t) for t in bad], good_results, f"task {at}")
        for at, change in ((1, (101, 100, 3)), (1, (100, 101, 3)), (4, (100, 100, 1024)), (2, (100, 97, 2)), (2, (97, 100, 2)), (0, (2, 2, 3)),
                           (3, (0, 0, 1))):
            bad = list(good_results)
            bad[at] = change + (100, 100)
            bad[5] = (100, 100, 2000, 100, 100)
            refused(good_tasks, bad, f"task {at}")
        refused(good_tasks, good_results, "table_budget", budget=63)
        ops, _ = ctx.edit_extend_script(ga, gb, task_array(good_tasks), result_array(good_results), 64)
        assert ops.size == 18
    finally:
        ga.free()
        gb.free()


def test_results_that_are_not_the_extension_are_refused(ctx):
    "edits off by +1 and by -1, and an N inside A': refused behind the launch, the smallest such task named, no ops"
    w, exp = refusal_world()
    good = [e[0] for e in exp]
    longer = World(np.random.default_rng(124))
    s = dna(longer.rng, 100)
    for q in range(4):
        longer.place(s.copy(), substituted(longer.rng, s, [20, 50, 80]), flags=(0, 7)[q % 2])
    exp_n = expected(longer, 6, 255)
    assert all(e[0] == (100, 100, 3, 100, 100) for e in exp_n)
    longer.rec_a[0][1][100 - 1 - 40] = N_[0]                  # (task 1 reads A backwards: offset 40 of A')
    longer.rec_b[0][3][10] = N_[0]                             # (task 3 complements B: an N stays an N)
    assert X.task_strings(*longer.records(), longer.tasks[1])[0][40] == N_[0] and X.task_strings(*longer.records(), longer.tasks[3])[1][89] == N_[0]

    def refused(world, results, named):
        ga, gb = world.upload(ctx)
        p, m = ctypes.c_void_p(0), ctypes.c_uint64(7)
        tk, rs = task_array(world.tasks), result_array(results)
        try:
            launches = ctx.timing("edit_extend_script")[1]
            rc = ctx.lib.nts_edit_extend_script(ctx.h, ga.h, gb.h, tk.ctypes.data, tk.size, rs.ctypes.data, 0, ctypes.byref(p), ctypes.byref(m), None)
            message = ctx.lib.nts_last_error(ctx.h).decode()
            assert ctx.timing("edit_extend_script")[1] == launches + 1
        finally:
            ga.free()
            gb.free()
        assert rc == -22 and f"results is not the extension of task {named}" in message and message.endswith(str(named)), (rc, message)
        assert p.value is None and m.value == 0
    for delta in (1, -1):
        bad = list(good)
        for at in (2, 5):
            bad[at] = (100, 100, 3 + delta, 100, 100)
        refused(w, bad, 2)
    refused(longer, [e[0] for e in exp_n], 1)

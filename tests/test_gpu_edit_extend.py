"""The free-end extension (csrc/nts_edit_extend.inc, nts_edit_extend) against the definition of tests/extend_brute.py, all five fields
of every task compared, on a small uploaded genome pair of two records each: identical strings of different lengths, a planted
breakpoint at offsets around the wave size, winners that need exactly 31 .. 129 edits (the rows where a row's lanes stride once, twice
and four times), single indels of 1 - 40 bases with and without substitutions beside them, the edit limit (the winner at exactly E, and
one that would need E + 1) at E = 1, 63, 64, 65 and 1023, penalties 3, 6 and 255, ties between cells of equal score, strings of no
and of one base, invalid bases at the first, a middle and the last position of either string and beyond the winner, all eight
combinations of the three flags, strings that end at the first base of the first record, at the last base of the last record and at a
record seam, 2 000 random tasks, no task (by the timer: no launch), the refused arguments (the output untouched), the same bytes twice.
Every case is built and its expected results asserted on the CPU (case_* functions) before the GPU is called.  Every test runs under a
time limit of its own."""
import faulthandler

import numpy as np
import pytest

from tests import extend_brute as X

pytestmark = pytest.mark.gpu
STEP_SECONDS = 600
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
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


def dna(rng, n):
    return LETTERS[rng.integers(0, 4, size=n)]


def substituted(rng, s, places):
    out = s.copy()
    for at in places:
        out[at] = rng.choice(LETTERS[LETTERS != out[at]])
    return out


def unlike(rng, s):
    "a string of the length of s that differs from it at every base"
    return substituted(rng, s, range(s.size))


class World:
    """two genomes of two records each, grown string by string: place() stores a pair of strings so that reading them with the
    task's flags gives them back, and notes the task"""

    def __init__(self, rng):
        self.rng = rng
        self.rec_a, self.rec_b = [[], []], [[], []]
        self.tasks = []

    @staticmethod
    def _at(rec):
        return sum(p.size for p in rec)

    def place(self, sa, sb, flags=0, rec=0, n=None, m=None):
        "the task that reads sa from genome A and sb from genome B (n / m: ask for fewer bases); returns its index"
        stored_a = sa[::-1] if flags & X.A_BACKWARDS else sa
        stored_b = X.complement(sb) if flags & X.B_COMPLEMENT else sb
        stored_b = stored_b[::-1] if flags & X.B_BACKWARDS else stored_b
        at_a, at_b = self._at(self.rec_a[rec]), self._at(self.rec_b[rec])
        self.rec_a[rec].append(stored_a)
        self.rec_b[rec].append(stored_b)
        pos_a = at_a + (sa.size - 1 if flags & X.A_BACKWARDS and sa.size else 0)
        pos_b = at_b + (sb.size - 1 if flags & X.B_BACKWARDS and sb.size else 0)
        self.tasks.append((rec, pos_a, sa.size if n is None else n, rec, pos_b, sb.size if m is None else m, flags))
        return len(self.tasks) - 1

    def filler(self, rec, n):
        self.rec_a[rec].append(dna(self.rng, n))
        self.rec_b[rec].append(dna(self.rng, n))

    def records(self):
        return [[np.concatenate(r) if r else np.zeros(0, np.uint8) for r in recs] for recs in (self.rec_a, self.rec_b)]

    def expected(self, penalty, max_edits):
        "[(the five fields, cells of the largest score)] of the brute force over the tasks as read from the records"
        ra, rb = self.records()
        return [X.extend_brute(*X.task_strings(ra, rb, t), penalty, max_edits) for t in self.tasks]

    def upload(self, ctx):
        from ntsynt_amd.device import Genome
        out = []
        for parts in self.records():
            lens = np.array([p.size for p in parts], dtype=np.uint64)
            offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            out.append(Genome(ctx, ["r1", "r2"], np.concatenate(parts), offs, lens))
        return out


def task_array(tasks):
    from ntsynt_amd.device import TASK_DTYPE
    arr = np.zeros(len(tasks), dtype=TASK_DTYPE)
    for q, (rec_a, pos_a, n, rec_b, pos_b, m, flags) in enumerate(tasks):
        arr[q] = (pos_a, pos_b, rec_a, rec_b, n, m, flags, 0)
    return arr


def run(ctx, case, what):
    "case = (world, P, E, expected): the call, twice, against the expected fields"
    from ntsynt_amd.device import EXTEND_DTYPE
    world, penalty, max_edits, exp = case
    ga, gb = world.upload(ctx)
    try:
        arr = task_array(world.tasks)
        launches = ctx.timing("edit_extend")[1]
        got = ctx.edit_extend(ga, gb, arr, penalty, max_edits)
        launched = ctx.timing("edit_extend")[1] - launches
        again = ctx.edit_extend(ga, gb, arr, penalty, max_edits)
    finally:
        ga.free()
        gb.free()
    assert got.dtype == EXTEND_DTYPE and got.shape == (len(world.tasks),)
    want = [e[0] for e in exp]
    bad = [q for q, (g, e) in enumerate(zip(got.tolist(), want)) if tuple(g) != e][:5]
    print(f"{what}: P {penalty}, E {max_edits}, {len(world.tasks)} tasks, {sum(e[1] > 1 for e in exp)} with a tie, largest edits "
          f"{max([e[2] for e in want], default=0)}; first differences {bad}")
    assert not bad, (what, [(q, world.tasks[q], tuple(got[q]), want[q]) for q in bad])
    assert got.tobytes() == again.tobytes(), what
    assert launched == (1 if world.tasks else 0), (what, "launches of k_edit_extend", launched)


# ---- the cases: built and checked on the CPU

def case_identical():
    "identical strings of different lengths: the extension reaches the end of the shorter one with no edit"
    rng = np.random.default_rng(1)
    w = World(rng)
    s = dna(rng, 700)
    lengths = [(300, 340), (340, 300), (64, 65), (1, 2), (700, 129)]
    for n, m in lengths:
        w.place(s[:n], s[:m])
    exp = w.expected(6, 255)
    for (n, m), (e, _) in zip(lengths, exp):
        assert e == (min(n, m), min(n, m), 0, n, m), (n, m, e)
    return w, 6, 255, exp


BREAKS = (1, 63, 64, 65, 500)


def case_breakpoint(flags):
    "a common start of 1 .. 500 bases, then unrelated sequence: the extension ends at the breakpoint or a few chance matches behind it"
    rng = np.random.default_rng(2)
    w = World(rng)
    for at in BREAKS:
        s = dna(rng, at)
        tail = dna(rng, 300)
        other = np.concatenate([unlike(rng, tail[:1]), dna(rng, 299)])
        w.place(np.concatenate([s, tail]), np.concatenate([s, other]), flags=flags, rec=at % 2)
    exp = w.expected(6, 255)
    for at, (e, _) in zip(BREAKS, exp):
        assert at <= e[0] <= at + 16 and at <= e[1] <= at + 16 and e[3:] == (at + 300, at + 300), (at, e)
    assert any(e[0][:3] == (at, at, 0) for at, e in zip(BREAKS, exp))
    return w, 6, 255, exp


ROWS = (31, 32, 33, 63, 64, 65, 127, 128, 129)


def case_rows():
    "substitutions 20 bases apart up to the strings' common end: the winner is the end cell, with exactly 31 .. 129 edits"
    rng = np.random.default_rng(3)
    w = World(rng)
    for q, edits in enumerate(ROWS):
        s = dna(rng, 20 * edits + 15)
        w.place(s, substituted(rng, s, [10 + 20 * x for x in range(edits)]), flags=(0, 3, 6)[q % 3], rec=q % 2)
    exp = w.expected(6, 255)
    for edits, (e, _) in zip(ROWS, exp):
        assert e == (20 * edits + 15,) * 2 + (edits,) + (20 * edits + 15,) * 2, (edits, e)
    return w, 6, 255, exp


def case_indels():
    "one insertion or deletion of 1 .. 40 bases 150 bases into the flank, bare and with a substitution on either side: all crossed"
    rng = np.random.default_rng(4)
    w = World(rng)
    want = []
    for n in range(1, 41):
        s = dna(rng, 400)
        ins = np.concatenate([s[:150], dna(rng, n), s[150:]])
        both = substituted(rng, ins, [60, 150 + n + 120])
        for a, b, edits in ((s, ins, n), (ins, s, n), (s, both, n + 2), (both, s, n + 2)):
            w.place(a, b, rec=n % 2)
            want.append((a.size, b.size, edits, a.size, b.size))
    exp = w.expected(6, 255)
    assert [e[0] for e in exp] == want, [(q, e[0], x) for q, (e, x) in enumerate(zip(exp, want)) if e[0] != x][:5]
    return w, 6, 255, exp


def case_limit(max_edits):
    """substitutions `step` bases apart: E of them and the common end (the winner at exactly E), and E + 1 of them (the winner is the best
    within E: the cell in front of the last substitution)"""
    rng = np.random.default_rng(500 + max_edits)
    penalty, step = (3, 4) if max_edits > 129 else (6, 8)
    w = World(rng)
    s = dna(rng, step * (max_edits + 1) + step - 1)
    places = [step - 1 + step * x for x in range(max_edits + 1)]
    w.place(s[:places[-1]], substituted(rng, s, places[:-1])[:places[-1]])
    w.place(s, substituted(rng, s, places), flags=3)
    exp = w.expected(penalty, max_edits)
    assert exp[0][0] == (places[-1], places[-1], max_edits, places[-1], places[-1]), exp[0]
    assert exp[1][0] == (places[-1], places[-1], max_edits, s.size, s.size), exp[1]
    return w, penalty, max_edits, exp


def case_penalty(penalty):
    "a substitution with 100 and with 200 matches behind it: worth crossing at P = 3 and 6; at P = 255 only the second (2 * 200 > 253)"
    rng = np.random.default_rng(6)
    w = World(rng)
    s = dna(rng, 251)
    w.place(s[:151], substituted(rng, s[:151], [50]))
    w.place(s, substituted(rng, s, [50]), rec=1)
    exp = w.expected(penalty, 255)
    assert exp[0][0][:3] == ((50, 50, 0) if penalty == 255 else (151, 151, 1)) and exp[1][0][:3] == (251, 251, 1), (penalty, exp)
    return w, penalty, 255, exp


def case_ties():
    """P = 4, a substitution with exactly one match behind it: stopping in front of it scores the same, and the fewer edits win.  P = 3,
    `AC` repeated against `CA` repeated behind a common start: dropping A's first base and skipping B's first base score the same with
    one edit each, and the smaller d = j - i wins."""
    rng = np.random.default_rng(7)
    w = World(rng)
    s = np.concatenate([dna(rng, 40), LETTERS[[2]]])         # (ends with G)
    w.place(np.concatenate([s, LETTERS[[0, 1]]]), np.concatenate([s, LETTERS[[3, 1]]]))
    exp4 = w.expected(4, 255)
    assert exp4[0][0][:3] == (41, 41, 0) and exp4[0][1] > 1, exp4
    v = World(rng)
    ac, ca = np.tile(LETTERS[[0, 1]], 10), np.tile(LETTERS[[1, 0]], 10)
    for flags in (0, 3):
        v.place(np.concatenate([s, ac]), np.concatenate([s, ca]), flags=flags)
    exp3 = v.expected(3, 255)
    for e, cells in exp3:
        assert e[:3] == (61, 60, 1) and cells > 1, exp3
    return (w, 4, 255, exp4), (v, 3, 255, exp3)


def case_short():
    "n = 0, m = 0, both, one base against many (the base at the start, further in, absent), asking for fewer bases than there are"
    rng = np.random.default_rng(8)
    w = World(rng)
    s = dna(rng, 50)
    none = np.zeros(0, np.uint8)
    one = LETTERS[[1]]
    many = np.concatenate([one, np.tile(LETTERS[[0]], 60)])
    late = np.concatenate([np.tile(LETTERS[[0]], 2), one, np.tile(LETTERS[[0]], 60)])
    for a, b in ((none, s), (s, none), (none, none), (one, many), (many, one), (one, late), (late, one), (one, many[1:]), (one, one.copy())):
        for flags in (0, 7):
            w.place(a, b, flags=flags, rec=flags & 1)
    w.place(s, s.copy(), n=0, m=7)
    w.place(s, s.copy(), n=20, m=50, flags=3)
    exp = w.expected(3, 10)
    want = [(0, 0, 0, 0, 50), (0, 0, 0, 50, 0), (0, 0, 0, 0, 0), (1, 1, 0, 1, 61), (1, 1, 0, 61, 1), (0, 0, 0, 1, 63), (0, 0, 0, 63, 1),
            (0, 0, 0, 1, 60), (1, 1, 0, 1, 1)]
    assert [e[0] for e in exp] == [x for x in want for _ in (0, 1)] + [(0, 0, 0, 0, 7), (20, 20, 0, 20, 50)], exp
    return w, 3, 10, exp


def case_invalid():
    """an N at the first, a middle and the last position of either string, and one beyond the winner (only valid_* changes): 200
    identical bases, then unrelated ones"""
    rng = np.random.default_rng(9)
    w = World(rng)
    s = dna(rng, 200)
    a, b = np.concatenate([s, dna(rng, 100)]), np.concatenate([s, dna(rng, 100)])
    b[200] = unlike(rng, a[200:201])[0]

    def with_n(x, at):
        return np.concatenate([x[:at], N_, x[at + 1:]])
    spots = (0, 100, 299, 280)
    for flags in (0, 7):
        w.place(a, b, flags=flags)
        for at in spots:
            w.place(with_n(a, at), b, flags=flags, rec=1)
            w.place(a, with_n(b, at), flags=flags)
            w.place(with_n(a, at), with_n(b, at), flags=flags, rec=1)
    exp = w.expected(6, 255)
    for half in (0, 13):
        clean = exp[half][0]
        assert 200 <= clean[0] <= 216 and clean[3:] == (300, 300), clean
        for q, at in enumerate(spots):
            ea, eb, eab = (exp[half + 1 + 3 * q + x][0] for x in range(3))
            assert ea[3:] == (at, 300) and eb[3:] == (300, at) and eab[3:] == (at, at), (at, ea, eb, eab)
            if at >= 280:                                     # beyond the winner: only valid_* changes
                assert ea[:3] == eb[:3] == eab[:3] == clean[:3], (at, ea, eb, eab, clean)
            else:
                assert ea[0] == eb[1] == eab[0] == eab[1] == at and ea[2] == eb[2] == eab[2] == 0, (at, ea, eb, eab)
    return w, 6, 255, exp


def case_directions():
    "one pair of strings under all eight combinations of the three flags: eight equal results"
    rng = np.random.default_rng(10)
    w = World(rng)
    s = dna(rng, 260)
    a = np.concatenate([s, dna(rng, 40)])
    b = np.concatenate([substituted(rng, np.concatenate([s[:90], dna(rng, 7), s[90:]]), [30, 200]), dna(rng, 40)])
    for flags in range(8):
        w.filler(flags & 1, 5)
        w.place(a, b, flags=flags, rec=flags & 1)
    exp = w.expected(6, 255)
    assert all(e == exp[0] for e in exp) and exp[0][0][2] == 9 and exp[0][0][0] >= 260, exp
    return w, 6, 255, exp


def case_record_limits():
    """a backwards string that ends at base 0 of record 0, a forwards one that ends at the last base of the last record, strings that
    touch the seam between the records from both sides -- in either genome"""
    rng = np.random.default_rng(11)
    w = World(rng)
    s = dna(rng, 120)
    t = substituted(rng, s, [70])
    first = w.place(s, t, flags=3, rec=0)                     # both backwards, down to base 0 of record 0
    w.filler(0, 9)
    seam_left = w.place(s, t, flags=0, rec=0)                 # forwards, up to the last base of record 0
    seam_right = w.place(s, t, flags=3, rec=1)                # backwards, down to base 0 of record 1
    w.filler(1, 9)
    last = w.place(s, t, flags=0, rec=1)                      # forwards, up to the last base of record 1: the genome's last base
    (ra, rb) = w.records()
    assert w.tasks[first][1] == 119 and w.tasks[first][4] == 119 and w.tasks[seam_right][1] == 119
    assert w.tasks[seam_left][1] + 120 == ra[0].size == rb[0].size and w.tasks[last][1] + 120 == ra[1].size == rb[1].size
    # and across: A at a record's end against B in the middle of its record, and the other way round
    w.tasks.append((0, w.tasks[seam_left][1], 120, 1, w.tasks[seam_right][4], 120, 2))
    w.tasks.append((1, 119, 120, 0, w.tasks[seam_left][4], 120, 1))
    exp = w.expected(6, 255)
    assert all(e[0] == (120, 120, 1, 120, 120) for e in exp), exp
    return w, 6, 255, exp


def legal(size, n, backwards):
    "the first and the last position from which n bases of a record of `size` bases can be read"
    if n == 0:
        return 0, size
    return (n - 1, size - 1) if backwards else (0, size - n)


def case_random(penalty, max_edits, seed):
    """500 tasks with n, m <= 200 and mixed flags over records of which genome B holds a mutated copy (record 0) and a mutated reverse
    complement (record 1), a few N among them: related strings for matching flags, unrelated ones for the others"""
    rng = np.random.default_rng(seed)
    w = World(rng)
    size = 6000
    for rec in (0, 1):
        a = dna(rng, size)
        b = substituted(rng, a, np.flatnonzero(rng.random(size) < 0.04))
        a[rng.integers(0, size, 6)] = ord("N")
        b[rng.integers(0, size, 6)] = ord("N")
        w.rec_a[rec].append(a)
        w.rec_b[rec].append(X.complement(b)[::-1] if rec else b)
    for _ in range(500):
        rec = int(rng.integers(0, 2))
        n, m = int(rng.integers(0, 201)), int(rng.integers(0, 201))
        flags = int(rng.integers(0, 8)) if rng.random() < 0.3 else int(rng.choice([0, 3]) if rec == 0 else rng.choice([6, 1]))
        (lo_a, hi_a), (lo_b, hi_b) = legal(size, n, flags & X.A_BACKWARDS), legal(size, m, flags & X.B_BACKWARDS)
        pos_a = int(rng.integers(lo_a, hi_a + 1))
        mirror = size - 1 - pos_a if rec else pos_a           # where record B holds the base that A has at pos_a
        pos_b = mirror + int(rng.integers(-2, 3)) * int(rng.random() < 0.3)
        w.tasks.append((rec, pos_a, n, int(rng.integers(0, 2)) if rng.random() < 0.05 else rec, min(max(pos_b, lo_b), hi_b), m, flags))
    exp = w.expected(penalty, max_edits)
    assert sum(e[0][2] >= 3 for e in exp) >= 20 and sum(e[0][0] == e[0][3] for e in exp) >= 50 and sum(e[1] > 1 for e in exp) >= 5
    assert sum(e[0][3] < t[2] or e[0][4] < t[5] for e, t in zip(exp, w.tasks)) >= 5
    return w, penalty, max_edits, exp


# ---- the tests

def test_identical_strings_reach_the_end(ctx):
    run(ctx, case_identical(), "identical strings")


@pytest.mark.parametrize("flags", [0, 7])
def test_planted_breakpoint(ctx, flags):
    run(ctx, case_breakpoint(flags), f"breakpoints, flags {flags}")


def test_rows_where_the_lane_strides_change(ctx):
    run(ctx, case_rows(), "winners with 31 .. 129 edits")


def test_single_indels_of_1_to_40_bases(ctx):
    run(ctx, case_indels(), "indels")


@pytest.mark.parametrize("max_edits", [1, 63, 64, 65, 1023])
def test_edit_limit(ctx, max_edits):
    run(ctx, case_limit(max_edits), f"edit limit {max_edits}")


@pytest.mark.parametrize("penalty", [3, 6, 255])
def test_penalty(ctx, penalty):
    run(ctx, case_penalty(penalty), f"penalty {penalty}")


def test_ties_go_to_fewer_edits_then_to_the_smaller_diagonal(ctx):
    for case in case_ties():
        run(ctx, case, "ties")


def test_short_strings(ctx):
    run(ctx, case_short(), "short strings")


def test_invalid_bases_cut_the_strings(ctx):
    run(ctx, case_invalid(), "invalid bases")


def test_all_eight_directions(ctx):
    run(ctx, case_directions(), "directions")


def test_record_limits_and_seams(ctx):
    run(ctx, case_record_limits(), "record limits")


@pytest.mark.parametrize("penalty,max_edits,seed", [(3, 20, 21), (6, 255, 22), (4, 64, 23), (12, 1023, 24)])
def test_random_tasks(ctx, penalty, max_edits, seed):
    run(ctx, case_random(penalty, max_edits, seed), f"500 random tasks, seed {seed}")


def test_no_task_launches_nothing(ctx):
    rng = np.random.default_rng(30)
    w = World(rng)
    w.filler(0, 10)
    w.filler(1, 10)
    before = ctx.timing("edit_extend")[1]
    run(ctx, (w, 6, 255, []), "no task")
    assert ctx.timing("edit_extend")[1] == before


def test_refused_arguments_leave_the_output_untouched(ctx):
    from ntsynt_amd.device import EXTEND_DTYPE, NtsError
    rng = np.random.default_rng(31)
    w = World(rng)
    s = dna(rng, 100)
    w.place(s, s.copy())
    w.filler(0, 5)
    w.place(s, s.copy(), rec=1)
    good = [(0, 0, 100, 0, 0, 100, 0), (1, 99, 100, 1, 99, 100, 3), (0, 105, 0, 1, 100, 0, 3)]    # (the last: n = m = 0 at pos = the record's length)
    ga, gb = w.upload(ctx)

    def refused(tasks, penalty=6, max_edits=255):
        out = np.full(len(tasks), 0xAB, dtype=np.uint8).repeat(EXTEND_DTYPE.itemsize).view(EXTEND_DTYPE)
        with pytest.raises(NtsError) as err:
            ctx.edit_extend(ga, gb, task_array(tasks), penalty, max_edits, out=out)
        assert "code -22" in str(err.value), err.value
        assert out.tobytes() == b"\xab" * out.nbytes, "a refused call wrote to the output"
    try:
        got = ctx.edit_extend(ga, gb, task_array(good), 6, 255)
        assert got.tolist() == [(100, 100, 0, 100, 100), (100, 100, 0, 100, 100), (0, 0, 0, 0, 0)]
        for penalty, max_edits in ((2, 255), (0, 255), (256, 255), (6, 0), (6, 1024)):
            refused(good, penalty, max_edits)
        for at, field, value in ((0, 2, 65536), (0, 5, 65536), (1, 6, 8), (1, 6, 1 << 31), (0, 0, 2), (0, 3, 2),
                                 (0, 2, 106), (0, 1, 6), (0, 5, 106), (0, 4, 6),       # forwards: pos + n > the record's length
                                 (1, 1, 98), (1, 4, 98), (1, 2, 101),                  # backwards: n > pos + 1
                                 (1, 1, 100), (1, 4, 100),                             # backwards from beyond the last base
                                 (2, 1, 106), (2, 4, 101)):                            # n = 0 beyond pos = the record's length
            bad = [list(t) for t in good]
            bad[at][field] = value
            refused([tuple(t) for t in bad])
        with pytest.raises(ValueError):
            ctx.edit_extend(ga, gb, task_array(good), 6, 255, out=np.zeros(2, dtype=EXTEND_DTYPE))
    finally:
        ga.free()
        gb.free()

"""The shared wave body of the two table kernels (csrc/nts_edit_fr_script.inc, fr_script_wave) through both of its readers: the same
string pairs go to nts_edit_wide_script as segments (SegReader) and to nts_edit_extend_script as tasks over the same bases (TaskReader:
A forwards, B forwards, or for a flipped member backwards and complemented from the base the wide kernel starts at; results = the
member's lengths and its distance).  Op for op, `op`, `p`, `q`, `base_a` and `base_b` of the two calls are equal, and equal to the full
table and walk of tests/variants_brute.py.  The members, each unflipped and flipped: D = 1, 63, 64, 65 and 300 (the lane stride, the
row parity), one base against many (n = 1), a script that begins with an indel (the walk reaches row 0), and a match run of 64 and of
65 bases behind the last mismatch (the ballot's 64 positions).  The case is built and checked on the CPU before the GPU is called."""
import faulthandler

import numpy as np
import pytest

from tests import identity_brute as B
from tests import variants_brute as V
from tests.test_gpu_edit_segments import Pair, dna, substituted
from tests.test_gpu_edit_wide import add, inserted, segment_array
from tests.test_gpu_edit_wide_script import expected

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
BAND, MAX_EDITS = 31, 1023
FIELDS = ("op", "p", "q", "base_a", "base_b")
WHAT = ("D 1", "D 63", "D 64", "D 65", "D 300", "n 1", "begins with an indel", "64 matches behind the last mismatch", "65 matches behind the last mismatch")
DISTANCES = (1, 63, 64, 65, 300, 39, 40, 41, 41)


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def members_of(p, rng, flip):
    "the nine members of WHAT as nine intervals of one segment each"
    s = dna(rng, 200)
    add(p, [(s, substituted(rng, s, [100]))], flip=flip, margin=(3, 2), kinds=[B.OFFBAND])       # (offband by hand: D = 1 is no member otherwise)
    s = dna(rng, 200)
    add(p, [(s, inserted(rng, s, 90, 63))], flip=flip, margin=(1, 4))
    s = dna(rng, 260)
    add(p, [(s, substituted(rng, s, range(2, 258, 4)))], flip=flip, margin=(2, 2))               # 64 substitutions: a candidate beyond the band
    s = dna(rng, 200)
    add(p, [(inserted(rng, s, 110, 65), s)], flip=flip, margin=(0, 3), rec=1)
    s = dna(rng, 240)
    add(p, [(s, inserted(rng, s, 120, 300))], flip=flip, margin=(5, 0), rec=1)
    s = dna(rng, 40)
    add(p, [(s[17:18], s)], flip=flip, margin=(2, 2))
    s = dna(rng, 150)
    s[0] = ord("C")
    add(p, [(s, np.concatenate([np.full(40, ord("A"), np.uint8), s]))], flip=flip, margin=(4, 4))
    for run in (64, 65):
        s = dna(rng, 300)
        add(p, [(substituted(rng, s, [s.size - 1 - run]), inserted(rng, s, 20, 40))], flip=flip, margin=(1, 1), rec=1)


@pytest.fixture(scope="module")
def case():
    "(pair, expected(...)): made once, checked here, left unchanged"
    rng = np.random.default_rng(2024)
    p = Pair(rng)
    for flip in (False, True):
        members_of(p, rng, flip)
    exp = expected(p, BAND, MAX_EDITS)
    _, final, ops, first, members, strings = exp
    assert members == list(range(2 * len(WHAT))) and final == list(DISTANCES) * 2, final
    assert max(max(a.size, b.size) for a, b in strings.values()) <= 2000
    for half in (0, len(WHAT)):
        of = lambda q: ops[first[half + q]:first[half + q + 1]]                      # noqa: E731
        assert strings[half + 5][0].size == 1
        assert of(6)[0][1:4] == (0, 0, V.INS) and of(6)[1][1] == 0                   # the walk ends along row 0
        for q, run in ((7, 64), (8, 65)):
            n = strings[half + q][0].size
            assert of(q)[-1][1:4] == (n - 1 - run, n - 1 - run + 40, V.SUB)          # the last op, `run` equal bases behind it
    return p, exp


@pytest.fixture(scope="module")
def scripts(case):
    "the ops of both calls, per member: ({member: ops of nts_edit_wide_script}, {member: ops of nts_edit_extend_script})"
    from ntsynt_amd.device import EXTEND_B_BACKWARDS, EXTEND_B_COMPLEMENT, EXTEND_DTYPE, TASK_DTYPE, Context
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    pair, (narrow, final, _, first, members, _) = case
    ctx = Context(0)
    (ga, _, _), (gb, _, _) = pair.upload(ctx)
    try:
        arr = segment_array(pair)
        _, dist = ctx.edit_segments(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, BAND, with_distances=True)
        _, got_final = ctx.edit_wide(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, BAND, MAX_EDITS, dist)
        assert dist.tolist() == narrow and got_final.tolist() == final
        wide, wide_first = ctx.edit_wide_script(ga, gb, pair.iv_a, pair.iv_b, arr, pair.flip, BAND, MAX_EDITS, got_final)
        tasks, results = np.zeros(len(members), dtype=TASK_DTYPE), np.zeros(len(members), dtype=EXTEND_DTYPE)
        for t, i in enumerate(members):
            iv, x, dx, y, dy, _ = pair.segs[i]
            (rec_a, start_a, _), (rec_b, start_b, end_b) = pair.iv_a[iv], pair.iv_b[iv]
            flipped = bool(pair.flip[iv])
            pos_b = start_b + (end_b - start_b - 1 - y) if flipped else start_b + y        # the base the wide kernel starts at
            tasks[t] = (start_a + x, pos_b, rec_a, rec_b, dx, dy, (EXTEND_B_BACKWARDS | EXTEND_B_COMPLEMENT) if flipped else 0, 0)
            results[t] = (dx, dy, final[i], dx, dy)
        ext, ext_first = ctx.edit_extend_script(ga, gb, tasks, results)
    finally:
        ga.free()
        gb.free()
        ctx.close()
        faulthandler.cancel_dump_traceback_later()
    assert wide_first.tolist() == first and ext_first.tolist() == [first[i] for i in members] + [first[-1]]
    of_wide = {i: wide[int(wide_first[i]):int(wide_first[i + 1])] for i in members}
    of_ext = {i: ext[int(ext_first[t]):int(ext_first[t + 1])] for t, i in enumerate(members)}
    for t, i in enumerate(members):
        assert (of_wide[i]["seg"] == i).all() and (of_ext[i]["seg"] == t).all()
    return of_wide, of_ext


@pytest.mark.parametrize("flipped", (False, True), ids=("unflipped", "flipped"))
@pytest.mark.parametrize("which", range(len(WHAT)), ids=[w.replace(" ", "_") for w in WHAT])
def test_both_readers_give_the_canonical_script(case, scripts, which, flipped):
    _, (_, final, ops, first, _, strings) = case
    of_wide, of_ext = scripts
    i = which + (len(WHAT) if flipped else 0)
    a, b = strings[i]
    brute = [(op, p, q, base_a, base_b) for _, p, q, op, base_a, base_b in ops[first[i]:first[i + 1]]]        # (variants_brute.op_records)
    got_wide = [tuple(int(o[f]) for f in FIELDS) for o in of_wide[i]]
    got_ext = [tuple(int(o[f]) for f in FIELDS) for o in of_ext[i]]
    print(f"{WHAT[which]}, flipped {flipped}: n {a.size}, m {b.size}, D {final[i]}, {len(got_wide)} and {len(got_ext)} ops")
    assert len(brute) == final[i] == DISTANCES[which]
    assert got_wide == got_ext, [(q, w, e) for q, (w, e) in enumerate(zip(got_wide, got_ext)) if w != e][:5]
    assert got_wide == brute, [(q, w, e) for q, (w, e) in enumerate(zip(got_wide, brute)) if w != e][:5]

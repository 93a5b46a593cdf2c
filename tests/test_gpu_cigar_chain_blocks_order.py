"""nts_cigar_chain_blocks in the call order of docs/design/04_24_call_order.md: the call shares the staged index (the `cigx_*` buffers and
`ivs_tmp`) with cigar_lift, cigar_lift_stats, cigar_text and cigar_lift_pairs and follows cigar_build in every round, so in ONE context
it is made after and before each of the five, at rising and falling sizes, and every result must be byte-equal to the result of a fresh
context -- and the partner's to the catalogue's expectation (tests/call_order_cases.py, read only; for cigar_lift_pairs, which the
catalogue does not hold, to the brute force of tests/lift_pairs_brute.py)."""
import faulthandler

import pytest

from tests import call_order_cases as C
from tests import chain_brute as CB
from tests import lift_pairs_brute as PB
from tests.test_gpu_cigar_lift_pairs import random_world, ranges_of

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_lift", "cigar_lift_stats", "cigar_text", "cigar_lift_pairs")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def cases():
    "the call's input at S and L (four times S), its bytes from a context that made no other call, and the joined lift's ranges and records"
    from ntsynt_amd.device import Context
    out = {}
    for size, (seed, pairs, entries, ranges, most) in (("S", (51, 8, 20, 60, 3)), ("L", (52, 40, 80, 240, 5))):
        w, quads, want = random_world(seed, pairs, entries, ranges, most=most)
        ctx = Context(0)
        try:
            got = ctx.cigar_chain_blocks(*w[:4])
        finally:
            ctx.close()
        pairs_w, blocks_w = CB.brute_blocks(*w[:4])          # (the fresh context's bytes are the brute force's)
        assert list(zip(*(got[0][f].tolist() for f in ("a0", "a1", "b0", "b1", "eq", "x", "first_block", "n_blocks")))) == pairs_w, size
        assert list(zip(*(got[1][f].tolist() for f in ("size", "dt", "dq")))) == blocks_w and got[2].tobytes() == CB.brute_text(pairs_w, blocks_w)[0], size
        out[size] = (w[:4], tuple(g.tobytes() for g in got), ranges_of(quads), want)
    assert all(out["L"][0][i].size >= 4 * out["S"][0][i].size for i in (0, 1, 2)) and out["S"][1] != out["L"][1]
    return out


def partner_holds(ctx, cases, partner, size):
    if partner == "cigar_lift_pairs":
        args, _, ranges, want = cases[size]
        got = ctx.cigar_lift_pairs(*args, ranges)
        return list(zip(*(got[f].tolist() for f in PB.FIELDS))) == want
    return C.BY_NAME[partner].run(ctx, C.case_of(partner, size)) == C.expected_of(partner, size)


@pytest.mark.parametrize("partner", PARTNERS)
def test_after_and_before_every_reader_and_the_builder(cases, partner):
    from ntsynt_amd.device import Context
    ctx = Context(0)
    try:
        for step, (mine, theirs) in enumerate((("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))):
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "in front")
            args, fresh = cases[mine][:2]
            assert tuple(g.tobytes() for g in ctx.cigar_chain_blocks(*args)) == fresh, (step, mine, "behind", partner, theirs)
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "behind")
    finally:
        ctx.close()

"""nts_cigar_lift_pairs in the call order of docs/design/04_24_call_order.md: the call shares the staged index (the `cigx_*` buffers and
`ivs_tmp`) with cigar_lift, cigar_lift_stats and cigar_text and follows cigar_build in every round, so in ONE context it is made after
and before each of the four, at rising and falling sizes, and every result must be byte-equal to the result of a fresh context -- and
the partner's to the catalogue's expectation (tests/call_order_cases.py, read only)."""
import faulthandler

import pytest

from tests import call_order_cases as C
from tests import lift_pairs_brute as PB
from tests.test_gpu_cigar_lift_pairs import random_world, ranges_of

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_lift", "cigar_lift_stats", "cigar_text")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def cases():
    "the call's input at S and L (four times S) and its bytes from a context that made no other call"
    from ntsynt_amd.device import Context
    out = {}
    for size, (seed, pairs, entries, ranges, most) in (("S", (51, 8, 20, 60, 3)), ("L", (52, 40, 80, 240, 5))):
        w, quads, want = random_world(seed, pairs, entries, ranges, most=most)
        ctx = Context(0)
        try:
            got = ctx.cigar_lift_pairs(*w[:4], ranges_of(quads))
        finally:
            ctx.close()
        assert list(zip(*(got[f].tolist() for f in PB.FIELDS))) == want, size          # (the fresh context's bytes are the brute force's records)
        fresh = got.tobytes()
        out[size] = (w[:4] + (ranges_of(quads),), fresh)
    assert all(out["L"][0][i].size >= 4 * out["S"][0][i].size for i in (0, 1, 2, 4)) and out["S"][1] != out["L"][1]
    return out


@pytest.mark.parametrize("partner", PARTNERS)
def test_after_and_before_every_reader_and_the_builder(cases, partner):
    from ntsynt_amd.device import Context
    entry = C.BY_NAME[partner]
    ctx = Context(0)
    try:
        for step, (mine, theirs) in enumerate((("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))):
            assert entry.run(ctx, C.case_of(partner, theirs)) == C.expected_of(partner, theirs), (step, partner, theirs, "in front")
            args, fresh = cases[mine]
            assert ctx.cigar_lift_pairs(*args).tobytes() == fresh, (step, mine, "behind", partner, theirs)
            assert entry.run(ctx, C.case_of(partner, theirs)) == C.expected_of(partner, theirs), (step, partner, theirs, "behind")
    finally:
        ctx.close()

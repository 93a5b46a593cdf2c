"""nts_cigar_depth in the call order of docs/design/04_24_call_order.md: the call shares the staged index (the `cigx_*` buffers and
`ivs_tmp`, which it fetches a second time for its sort, reduction and scans) with the CIGAR readers, follows cigar_build and runs in a
context that has built a graph, so in ONE context it is made after and before each of them and nts_cigar_pad, at rising and falling
sizes, and every result must equal the brute force's (tests/conservation_brute.py) and the partner's the catalogue's expectation
(tests/call_order_cases.py, read only; nts_cigar_pad's, which the catalogue does not hold, tests/multi_maf_brute.py's)."""
import faulthandler

import pytest

from tests import call_order_cases as C
from tests import conservation_brute as CB
from tests import multi_maf_brute as MM
from tests.test_gpu_cigar_depth import as_tuples
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_lift", "cigar_lift_stats", "cigar_text", "graph_build", "cigar_pad")


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def cases():
    "the call's input at S and L (ten times the chains of S), the brute force's answer as lists, and nts_cigar_pad's for the same input"
    out = {}
    for size, (seed, n_chains, n_groups) in (("S", (71, 30, 6)), ("L", (72, 300, 40))):
        specs = random_groups(seed, n_chains, n_groups)
        cigar, recs, lists = arrays([s[2] for s in specs])
        chains = [(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)]
        out[size] = ((cigar, recs, at_of(specs), n_groups), CB.segments(chains, n_groups), [list(w) for w in MM.pad_all(chains, n_groups)])
    assert out["L"][0][0].size >= 4 * out["S"][0][0].size and len(out["S"][1][0]) > 10
    return out


def partner_holds(ctx, cases, partner, size):
    if partner == "cigar_pad":
        return [g.tolist() for g in ctx.cigar_pad(*cases[size][0])] == cases[size][2]
    return C.BY_NAME[partner].run(ctx, C.case_of(partner, size)) == C.expected_of(partner, size)


@pytest.mark.parametrize("partner", PARTNERS)
def test_after_and_before_every_reader_the_builder_the_padder_and_a_graph_build(cases, partner):
    from ntsynt_amd.device import Context
    ctx = Context(0)
    try:
        for step, (mine, theirs) in enumerate((("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))):
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "in front")
            args, (want, want_first), _ = cases[mine]
            segs, seg_first = ctx.cigar_depth(*args)
            assert as_tuples(segs) == want and seg_first.tolist() == want_first, (step, mine, "behind", partner, theirs)
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "behind")
    finally:
        ctx.close()

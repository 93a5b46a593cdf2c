"""nts_cigar_profile in the call order of docs/design/04_24_call_order.md: it shares the staged index (the `cigx_*` buffers and
`ivs_tmp`, which it fetches a second time for its sorts and its scan) with the CIGAR readers, follows cigar_build and runs in a context
that has built a graph, so in ONE context it is made after and before cigar_build, cigar_rows, cigar_pad, cigar_depth, cigar_alleles and
graph_build, at rising and falling sizes, with equal bytes each way, and every result must equal the brute force's
(tests/profile_brute.py) and the partner's its own expectation (tests/call_order_cases.py, read only, for cigar_build and graph_build;
tests/maf_brute.py, tests/multi_maf_brute.py, tests/conservation_brute.py and tests/variant_sites_brute.py for the four the catalogue
does not hold).  The case tables live in this file."""
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import conservation_brute as CB
from tests import multi_maf_brute as MM
from tests import profile_brute as PB
from tests import variant_sites_brute as VB
from tests.test_gpu_cigar_alleles import as_tuples as allele_tuples
from tests.test_gpu_cigar_depth import as_tuples as depth_tuples
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups
from tests.test_gpu_cigar_profile import made_up
from tests.test_gpu_cigar_rows import case as rows_case
from tests.test_gpu_cigar_text import World, random_specs

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_rows", "cigar_pad", "cigar_depth", "cigar_alleles", "graph_build")
SIZES = {"S": dict(groups=(91, 30, 6), specs=(92, 40, 6)), "L": dict(groups=(93, 300, 40), specs=(94, 400, 12))}
STEPS = (("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def grouped():
    "per size: nts_cigar_profile's input, the brute force's answer, and nts_cigar_pad's, nts_cigar_depth's and nts_cigar_alleles' for the same chains"
    out = {}
    for size, table in SIZES.items():
        seed, n_chains, n_groups = table["groups"]
        specs = random_groups(seed, n_chains, n_groups)
        cigar, recs, lists = arrays([s[2] for s in specs])
        chains = [(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)]
        refs, alts = made_up(lists, seed, b"ACG")
        out[size] = dict(args=(cigar, recs, at_of(specs)), ref=np.frombuffer(b"".join(refs), dtype=np.uint8), alt=np.frombuffer(b"".join(alts), dtype=np.uint8),
                         n_groups=n_groups, profile=PB.columns(chains, refs, alts, n_groups), alleles=VB.alleles(chains, alts, n_groups),
                         pad=[list(w) for w in MM.pad_all(chains, n_groups)], depth=CB.segments(chains, n_groups), bytes={})
    assert out["L"]["args"][0].size >= 4 * out["S"]["args"][0].size and len(out["S"]["profile"][0]) > 10
    return out


def partner_holds(ctx, world, grouped, spans, partner, size):
    g = grouped[size]
    if partner == "cigar_pad":
        return [x.tolist() for x in ctx.cigar_pad(*g["args"], g["n_groups"])] == g["pad"]
    if partner == "cigar_depth":
        segs, seg_first = ctx.cigar_depth(*g["args"], g["n_groups"])
        return (depth_tuples(segs), seg_first.tolist()) == g["depth"]
    if partner == "cigar_alleles":
        alleles, allele_first, carriers = ctx.cigar_alleles(*g["args"], g["alt"], g["n_groups"])
        return (allele_tuples(alleles), allele_first.tolist(), carriers.tolist()) == g["alleles"]
    if partner == "cigar_rows":
        row_a, row_b, _ = ctx.cigar_rows(*spans[size]["args"], *world.genomes)
        return (row_a.tobytes().decode(), row_b.tobytes().decode()) == spans[size]["rows"]
    return C.BY_NAME[partner].run(ctx, C.case_of(partner, size)) == C.expected_of(partner, size)


def profile_holds(ctx, grouped, size):
    g = grouped[size]
    cols, col_first = ctx.cigar_profile(*g["args"], g["ref"], g["alt"], g["n_groups"])
    same = g["bytes"].setdefault("first", (cols.tobytes(), col_first.tobytes())) == (cols.tobytes(), col_first.tobytes())   # equal bytes each way
    return same and (PB.as_tuples(cols), col_first.tolist()) == g["profile"]


@pytest.mark.parametrize("partner", PARTNERS)
def test_the_call_after_and_before_every_partner(grouped, partner):
    from ntsynt_amd.device import Context
    ctx = Context(0)
    world = World(ctx)
    try:
        spans = {}
        if partner == "cigar_rows":
            for size in SIZES:
                seed, n_chains, mean = SIZES[size]["specs"]
                cigar, recs, where, rows_a, rows_b = rows_case(world, random_specs(seed, n_chains, mean))
                spans[size] = dict(args=(cigar, recs, where), rows=("".join(rows_a), "".join(rows_b)))
        for step, (mine, theirs) in enumerate(STEPS):
            assert partner_holds(ctx, world, grouped, spans, partner, theirs), (step, partner, theirs, "in front")
            assert profile_holds(ctx, grouped, mine), (step, mine, "cigar_profile behind", partner, theirs)
            assert partner_holds(ctx, world, grouped, spans, partner, theirs), (step, partner, theirs, "behind")
            assert profile_holds(ctx, grouped, theirs) and profile_holds(ctx, grouped, mine), (step, "one behind the other", theirs, mine)
    finally:
        world.free()
        ctx.close()

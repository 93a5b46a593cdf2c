"""nts_cigar_var_bases and nts_cigar_alleles in the call order of docs/design/04_24_call_order.md: both share the staged index (the
`cigx_*` buffers and `ivs_tmp`, which nts_cigar_alleles fetches a second time for its sorts and its scan) with the CIGAR readers, follow
cigar_build and run in a context that has built a graph, so in ONE context each is made after and before cigar_build, cigar_rows,
cigar_pad, cigar_depth and graph_build, at rising and falling sizes, and every result must equal the brute force's
(tests/variant_sites_brute.py) and the partner's its own expectation (tests/call_order_cases.py, read only, for cigar_build and
graph_build; tests/maf_brute.py, tests/multi_maf_brute.py and tests/conservation_brute.py for the three the catalogue does not hold).
The case tables live in this file."""
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import conservation_brute as CB
from tests import multi_maf_brute as MM
from tests import variant_sites_brute as VB
from tests.test_gpu_cigar_alleles import as_tuples, made_up_alts
from tests.test_gpu_cigar_depth import as_tuples as depth_tuples
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_pad import at_of, random_groups
from tests.test_gpu_cigar_rows import case as rows_case
from tests.test_gpu_cigar_text import World, random_specs

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_rows", "cigar_pad", "cigar_depth", "graph_build")
SIZES = {"S": dict(groups=(81, 30, 6), specs=(82, 40, 6)), "L": dict(groups=(83, 300, 40), specs=(84, 400, 12))}
STEPS = (("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def grouped():
    "per size: nts_cigar_alleles' input, the brute force's answer, and nts_cigar_pad's and nts_cigar_depth's for the same chains"
    out = {}
    for size, table in SIZES.items():
        seed, n_chains, n_groups = table["groups"]
        specs = random_groups(seed, n_chains, n_groups)
        cigar, recs, lists = arrays([s[2] for s in specs])
        chains = [(g, t0, lists[c]) for c, (g, t0, _) in enumerate(specs)]
        alts = made_up_alts(lists, seed, b"AC")
        out[size] = dict(args=(cigar, recs, at_of(specs)), alt=np.frombuffer(b"".join(alts), dtype=np.uint8), n_groups=n_groups,
                         alleles=VB.alleles(chains, alts, n_groups), pad=[list(w) for w in MM.pad_all(chains, n_groups)], depth=CB.segments(chains, n_groups))
    assert out["L"]["args"][0].size >= 4 * out["S"]["args"][0].size and len(out["S"]["alleles"][0]) > 10
    return out


def spanned(world, size):
    "per size: nts_cigar_var_bases' and nts_cigar_rows' input over the world's genomes and both expectations"
    seed, n_chains, mean = SIZES[size]["specs"]
    cigar, recs, spans, rows_a, rows_b = rows_case(world, random_specs(seed, n_chains, mean))
    lists = [cigar[int(r["first"]):int(r["first"] + r["n_cig"])].tolist() for r in recs]
    both = [VB.variant_bytes(entries, a, b) for entries, a, b in zip(lists, rows_a, rows_b)]
    return dict(args=(cigar, recs, spans), rows=("".join(rows_a), "".join(rows_b)), ref="".join(b[0] for b in both), alt="".join(b[1] for b in both),
                firsts=[np.concatenate(([0], np.cumsum([len(b[k]) for b in both]))).tolist() for k in (0, 1)])


def partner_holds(ctx, world, grouped, spans, partner, size):
    if partner == "cigar_pad":
        return [g.tolist() for g in ctx.cigar_pad(*grouped[size]["args"], grouped[size]["n_groups"])] == grouped[size]["pad"]
    if partner == "cigar_depth":
        segs, seg_first = ctx.cigar_depth(*grouped[size]["args"], grouped[size]["n_groups"])
        return (depth_tuples(segs), seg_first.tolist()) == grouped[size]["depth"]
    if partner == "cigar_rows":
        row_a, row_b, _ = ctx.cigar_rows(*spans[size]["args"], *world.genomes)
        return (row_a.tobytes().decode(), row_b.tobytes().decode()) == spans[size]["rows"]
    return C.BY_NAME[partner].run(ctx, C.case_of(partner, size)) == C.expected_of(partner, size)


def alleles_hold(ctx, grouped, size):
    g = grouped[size]
    alleles, allele_first, carriers = ctx.cigar_alleles(*g["args"], g["alt"], g["n_groups"])
    return (as_tuples(alleles), allele_first.tolist(), carriers.tolist()) == g["alleles"]


def var_bases_hold(ctx, world, spans, size):
    s = spans[size]
    ref, ref_first, alt, alt_first = ctx.cigar_var_bases(*s["args"], *world.genomes)
    return (ref.tobytes().decode(), alt.tobytes().decode(), [ref_first.tolist(), alt_first.tolist()]) == (s["ref"], s["alt"], s["firsts"])


@pytest.mark.parametrize("partner", PARTNERS)
def test_both_calls_after_and_before_every_partner(grouped, partner):
    from ntsynt_amd.device import Context
    ctx = Context(0)
    world = World(ctx)
    try:
        spans = {size: spanned(world, size) for size in SIZES}
        assert len(spans["L"]["ref"]) > 4 * len(spans["S"]["ref"]) > 40
        for step, (mine, theirs) in enumerate(STEPS):
            assert partner_holds(ctx, world, grouped, spans, partner, theirs), (step, partner, theirs, "in front")
            assert alleles_hold(ctx, grouped, mine), (step, mine, "cigar_alleles behind", partner, theirs)
            assert partner_holds(ctx, world, grouped, spans, partner, theirs), (step, partner, theirs, "between")
            assert var_bases_hold(ctx, world, spans, mine), (step, mine, "cigar_var_bases behind", partner, theirs)
            assert partner_holds(ctx, world, grouped, spans, partner, theirs), (step, partner, theirs, "behind")
            assert alleles_hold(ctx, grouped, theirs) and var_bases_hold(ctx, world, spans, theirs), (step, "one behind the other", theirs)
    finally:
        world.free()
        ctx.close()

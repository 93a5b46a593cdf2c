"""nts_cigar_rows in the call order of docs/design/04_24_call_order.md: the call shares the staged index (the `cigx_*` buffers and
`ivs_tmp`) with cigar_lift, cigar_lift_stats, cigar_text, cigar_lift_pairs and cigar_chain_blocks, follows cigar_build in every round and
runs in a context that has built a graph, so in ONE context it is made after and before each of them, at rising and falling sizes, and
every result must be byte-equal to the result of a fresh context -- which is the brute force's (tests/maf_brute.py) -- and the partner's
to the catalogue's expectation (tests/call_order_cases.py, read only; for cigar_lift_pairs and cigar_chain_blocks, which the catalogue
does not hold, to the brute forces of tests/lift_pairs_brute.py and tests/chain_brute.py)."""
import faulthandler

import numpy as np
import pytest

from tests import call_order_cases as C
from tests import chain_brute as CB
from tests import lift_pairs_brute as PB
from tests import maf_brute as MB
from tests.test_gpu_cigar_lift import arrays
from tests.test_gpu_cigar_lift_pairs import random_world, ranges_of
from tests.test_gpu_cigar_text import lengths_of, random_specs

pytestmark = pytest.mark.gpu
STEP_SECONDS = 300
PARTNERS = ("cigar_build", "cigar_lift", "cigar_lift_stats", "cigar_text", "cigar_lift_pairs", "cigar_chain_blocks", "graph_build")
RECORDS = ((2100, 1200, 1_000_000), (2300, 1300, 1_000_000))       # the records random_specs places its chains in


@pytest.fixture(autouse=True)
def step_time_limit():
    faulthandler.dump_traceback_later(STEP_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def upload(ctx, seqs):
    from ntsynt_amd.device import Genome
    sizes = np.array([len(s) for s in seqs], dtype=np.uint64)
    offs = np.concatenate(([0], np.cumsum(sizes[:-1]))).astype(np.uint64)
    return Genome(ctx, [f"r{i}" for i in range(len(seqs))], np.frombuffer("".join(seqs).encode(), dtype=np.uint8), offs, sizes)


@pytest.fixture(scope="module")
def cases():
    """the two genomes as strings; the call's input at S and L (five times S) with the brute force's rows, which a context that made no
    other call must give; and the inputs and records of the two partners the catalogue does not hold"""
    from ntsynt_amd.device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE, Context
    rng = np.random.default_rng(2902)
    seqs = [["".join("ACGTN"[v] for v in rng.choice(5, n, p=[0.245, 0.245, 0.245, 0.245, 0.02])) for n in lens] for lens in RECORDS]
    out = {"seqs": seqs}
    for size, (seed, n) in (("S", (43, 12)), ("L", (44, 60))):
        specs = random_specs(seed, n, 6)
        cigar, recs, lists = arrays([s[0] for s in specs])
        spans = np.zeros(len(specs), dtype=CIG_SPAN_DTYPE)
        rows = ([], [])
        for c, (_, ra, pa, rb, sb, back) in enumerate(specs):
            la, lb = lengths_of(lists[c])
            spans[c] = (pa, sb + lb - 1 if back and lb else sb, ra, rb, CIG_B_BACKWARDS if back else 0, 0)
            query = seqs[1][rb][sb:sb + lb]
            for row, made in zip(rows, MB.rows_from_cigar(lists[c], seqs[0][ra][pa:pa + la], MB.reverse_complement(query) if back else query)):
                row.append(made)
        first = np.concatenate(([0], np.cumsum([len(r) for r in rows[0]]))).astype(np.uint64)
        want = ("".join(rows[0]).encode(), "".join(rows[1]).encode(), first.tobytes())
        ctx = Context(0)
        try:
            genomes = [upload(ctx, s) for s in seqs]
            fresh = tuple(g.tobytes() for g in ctx.cigar_rows(cigar, recs, spans, *genomes))
            for g in genomes:
                g.free()
        finally:
            ctx.close()
        assert fresh == want, size
        out[size] = ((cigar, recs, spans), want)
    assert out["L"][0][0].size >= 4 * out["S"][0][0].size and out["S"][1] != out["L"][1]
    for size, (seed, pairs, entries, ranges, most) in (("S", (51, 8, 20, 60, 3)), ("L", (52, 40, 80, 240, 5))):
        w, quads, want = random_world(seed, pairs, entries, ranges, most=most)
        out["linked", size] = (w[:4], ranges_of(quads), want, CB.brute_blocks(*w[:4]))
    return out


def partner_holds(ctx, cases, partner, size):
    if partner == "cigar_lift_pairs":
        args, ranges, want, _ = cases["linked", size]
        got = ctx.cigar_lift_pairs(*args, ranges)
        return list(zip(*(got[f].tolist() for f in PB.FIELDS))) == want
    if partner == "cigar_chain_blocks":
        args, _, _, (pairs_w, blocks_w) = cases["linked", size]
        got = ctx.cigar_chain_blocks(*args)
        return list(zip(*(got[0][f].tolist() for f in ("a0", "a1", "b0", "b1", "eq", "x", "first_block", "n_blocks")))) == pairs_w and \
            list(zip(*(got[1][f].tolist() for f in ("size", "dt", "dq")))) == blocks_w and got[2].tobytes() == CB.brute_text(pairs_w, blocks_w)[0]
    return C.BY_NAME[partner].run(ctx, C.case_of(partner, size)) == C.expected_of(partner, size)


@pytest.mark.parametrize("partner", PARTNERS)
def test_after_and_before_every_reader_the_builder_and_a_graph_build(cases, partner):
    from ntsynt_amd.device import Context
    ctx = Context(0)
    try:
        genomes = [upload(ctx, s) for s in cases["seqs"]]
        for step, (mine, theirs) in enumerate((("S", "L"), ("L", "S"), ("S", "S"), ("L", "L"), ("S", "L"))):
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "in front")
            args, fresh = cases[mine]
            assert tuple(g.tobytes() for g in ctx.cigar_rows(*args, *genomes)) == fresh, (step, mine, "behind", partner, theirs)
            assert partner_holds(ctx, cases, partner, theirs), (step, partner, theirs, "behind")
        for g in genomes:
            g.free()
    finally:
        ctx.close()

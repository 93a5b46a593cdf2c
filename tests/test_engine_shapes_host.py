"""The hand-made graph shapes of tests/engine_shapes.py on the CPU: every case goes through the oracle (tests/engine_brute.py) and
must show the facts it was built for -- this ring yields no path, that walk visits more than 96 vertices, these two ends tie --
before a GPU sees it; the same scripts then run on the host-array engine (ntsynt_amd/synteny.py with its native walk, scan, degree
and bubble helpers), whose state must equal the oracle's after every call.  The random families must hold each feature the device
test relies on in at least 5 % of the families, on the oracle alone."""
import pytest

from tests import engine_shapes as ES

_TRACES = {}


def trace_of(name):
    if name not in _TRACES:
        case = ES.CASES[name]()
        _TRACES[name] = (case,) + ES.oracle_trace(case)
    return _TRACES[name]


@pytest.mark.parametrize("name", sorted(ES.CASES))
def test_case_shows_what_it_was_built_for(name):
    case, trace, br = trace_of(name)
    case["facts"](trace, br)


@pytest.mark.parametrize("name", sorted(ES.CASES))
def test_host_engine_equals_the_oracle_after_every_call(name):
    case, trace, _ = trace_of(name)
    twin = ES.Twin(case["G"], **case["par"])
    ES.same(trace, ES.play(twin, case["script"]), name)


def test_start_end_tie_is_settled_differently():
    """OPEN (docs/design/04_4_graph_stage.md): two path ends at the same position of two reference contigs.  The oracle starts at the end
    its component walk lists last, the engines at the smaller vertex id; ntJoin's determine_source_vertex is not part of the reference
    tree, so neither is pinned.  Where the last listed end is also the smaller id ("tie" in ES.CASES) all agree; here it is the larger
    one, and the engines walk the oracle's path backwards.  This test keeps the case and fails when either side changes its rule."""
    lay, hs = ES._tie(True)
    script = ES.FIRST(lay.lists)
    ora = ES.play(ES.OracleDriver(3, bp=ES.BIG, n=2), script)
    twin = ES.play(ES.Twin(3, bp=ES.BIG, n=2), script)
    assert hs[0] < hs[-1]
    assert ora[-1][1]["paths"] == [tuple(hs[::-1])] and twin[-1][1]["paths"] == [tuple(hs)]
    assert ora[1][2] == twin[1][2]                        # the graphs are the same up to the walk


def test_random_families_hold_every_feature_often_enough():
    n_fam = 300
    seen = dict.fromkeys(("ring", "branching", "bubble", "unoriented", "contig_change", "indel_cut", "small", "eroded"), 0)
    for seed in range(n_fam):
        case = ES.random_script(seed)
        d = ES.OracleDriver(case["G"], **case["par"])
        br = d.br
        ES.play(d, case["script"][:3])
        kinds = br.kinds()
        ES.play(d, case["script"][3:])
        info = br.ora.list_mx_info
        seen["ring"] += kinds["ring"] > 0
        seen["branching"] += kinds["branching"] > 0
        seen["bubble"] += br.counts["bubbles"] > 0
        seen["unoriented"] += br.counts["unoriented"] > 0
        seen["indel_cut"] += br.counts["indel_cuts"] > 0
        seen["small"] += br.counts["small"] > 0
        seen["eroded"] += br.counts["eroded"] > 0
        seen["contig_change"] += any(len({info[f][h][0] for h in p}) > 1 for p in br.paths for f in br.files)
        assert len(br.ora.list_mx_info[br.files[0]]) <= 800
    print(seen)
    assert all(v * 20 >= n_fam for v in seen.values()), seen


def test_host_engine_equals_the_oracle_on_the_random_families():
    "the random families of the device test, refinement round included, on the host-array engine"
    from tests import engine_brute as EB
    n_refined = 0
    for seed in range(300):
        case = ES.random_script(seed)
        d = ES.OracleDriver(case["G"], **case["par"])
        twin = ES.Twin(case["G"], **case["par"])
        ES.same(ES.play(d, case["script"]), ES.play(twin, case["script"]), f"family {seed}")
        if case["refine"] and d.br.blocks_:
            script = [("add", EB.refinement_lists(d.br, seed))] + ES.REFINE
            ES.same(ES.play(d, script), ES.play(twin, script), f"family {seed}: refinement")
            n_refined += 1
    assert n_refined >= 30

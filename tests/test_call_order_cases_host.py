"""The catalogue of tests/call_order_cases.py itself, on the CPU: every entry's expectation is there within seconds, L is four times S
in every dimension that sizes a scratch buffer, S and L expect different bytes, every case holds the outcomes that make it worth
running (asserted here, before any GPU is involved), the family table names scratch buffers that the sources really request, and the
long chain's seed leaves out no entry and no size."""
import os
import re
import time

import numpy as np
import pytest

from tests import call_order_cases as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ntsynt_amd", "csrc")
NAMES = [e.name for e in C.ENTRIES]
REQUIRED = ["edit_segments", "edit_wide", "edit_extend", "edit_script", "edit_wide_script", "edit_extend_script", "cigar_build", "cigar_lift",
            "cigar_lift_stats", "cigar_text", "iv_anchor_segments", "iv_links", "iv_sites", "iv_periods", "iv_period_hashes", "iv_families", "iv_family_sites", "hset_sweep", "hcount_capped",
            "minhash", "minhash_intervals", "bloom_insert", "engine_add_blocks"] + ["sketch_" + w for w in ("dense", "pruned_hi", "pruned_full", "tiers", "accept_list")]
NEW = ["fasta_parse", "graph_build", "graph_build_sliced", "bloom_insert_and", "bloom_cascade", "bloom_repeats", "bf_count_intervals", "bf_sample_intervals",
       "mx_screen", "minhash_pairs"]                          # the calls of every round
REQUIRED += NEW


def requested(files):
    "{scratch name: how often it is requested} in the given sources: the quoted first argument of ws_get / NTS_WS"
    out = {}
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            for name in re.findall(r'(?:ws_get\(ctx, |NTS_WS\([^"\n]*)"([a-z_0-9]+)"', fh.read()):
                out[name] = out.get(name, 0) + 1
    return out


def test_the_catalogue_holds_every_entry_the_design_section_names():
    assert set(REQUIRED) <= set(NAMES) and len(set(NAMES)) == len(NAMES)
    assert set(C.SOURCES) == set(NAMES) and C.HEAVY_PARTNER in NAMES and set(C.STAGED) <= set(NAMES)


def test_the_record_layouts_are_the_device_modules():
    from ntsynt_amd import device as D
    for mine, theirs in ((C.IDENTITY, D.IDENTITY_DTYPE), (C.OP, D.OP_DTYPE), (C.SEGMENT, D.SEGMENT_DTYPE), (C.EXTEND, D.EXTEND_DTYPE), (C.CHAIN, D.CHAIN_DTYPE),
                         (C.LIFT_HIT, D.LIFT_HIT_DTYPE), (C.LIFT_STATS, D.LIFT_STATS_DTYPE), (C.LINK, D.LINK_DTYPE), (C.SITE, D.SITE_DTYPE), (C.SAMPLE, D.SAMPLE_DTYPE)):
        assert mine == theirs


@pytest.mark.parametrize("name", NAMES)
def test_sizes_outcomes_and_time(name):
    e = C.BY_NAME[name]
    counts, exp = {}, {}
    for size in C.SIZES:
        t0 = time.perf_counter()
        case = C.case_of(name, size)
        exp[size] = C.expected_of(name, size)
        took = time.perf_counter() - t0
        counts[size] = e.counts(case)
        missing = [what for what, there in e.outcomes(case).items() if not there]
        print(f"{name} {size}: {counts[size]}, {len(exp[size])} expected bytes, {took:.2f} s")
        assert took < 5, (name, size, took)
        assert isinstance(exp[size], bytes) and len(exp[size]) > 0
        assert not missing, (name, size, "the case has no", missing)
        assert C.expected_of(name, size) is exp[size] and C.case_of(name, size) is case      # made once, left unchanged
    assert e.sizing and set(e.sizing) <= set(counts["S"])
    for dim in e.sizing:
        assert counts["S"][dim] > 0 and counts["L"][dim] >= 4 * counts["S"][dim], (name, dim, counts["S"][dim], counts["L"][dim])
    assert exp["S"] != exp["L"] and exp["S"] not in exp["L"]                                   # (a stale read cannot pass by chance)
    limit = {"S": (300, 20_000), "L": (300, 200_000)}
    for size in C.SIZES:
        case = C.case_of(name, size)
        if "bases" in counts[size]:
            assert counts[size]["bases"] <= limit[size][1], (name, size)
        if "pair" in case:
            assert max(s[2] for s in case["pair"].segs) <= 300 and max(s[4] for s in case["pair"].segs) <= 300
        if "world" in case:
            assert max(max(t[2], t[5]) for t in case["world"].tasks) <= 300


def test_the_edit_cases_hold_aligned_and_other_segments():
    "the `need=` of tests/test_gpu_edit_segments.py, for the whole family and both sizes"
    for size in C.SIZES:
        seen = C.pair_outcomes(C.case_of("edit_segments", size))
        assert all(seen.values()), (size, [k for k, v in seen.items() if not v])
        world = C.world_outcomes(C.case_of("edit_extend", size))
        assert all(world.values()), (size, world)


def test_family_table_against_the_sources():
    every = {name: requested(files) for name, files in C.SOURCES.items()}
    for e in C.ENTRIES:
        for ws in e.family:
            assert ws in every[e.name], (e.name, "does not request", ws)
        if e.ivs_tmp:
            assert "ivs_tmp" in every[e.name], e.name
    met = 0
    for x in C.ENTRIES:
        for y in C.ENTRIES:
            if x is not y and x.family & y.family:
                met += 1
                for ws in x.family & y.family:
                    assert ws in every[x.name] and ws in every[y.name], (x.name, y.name, ws)
    assert met >= 20
    # the shared names of docs/design/04_24_call_order.md are in the table, between the entry points it names
    for ws in ("edit_seg", "edit_ivs", "edit_dist", "edit_num"):
        assert all(ws in C.BY_NAME[n].family for n in ("edit_segments", "edit_wide", "edit_script", "edit_wide_script")), ws
    for ws in ("edit_num", "edit_first", "edit_kept", "edit_ops"):
        assert all(ws in C.BY_NAME[n].family for n in ("edit_script", "edit_wide_script", "edit_extend_script")), ws
    for ws in C.IVF_SHARED:
        assert all(ws in C.BY_NAME[n].family for n in ("iv_period_hashes", "iv_families", "iv_family_sites")), ws
        assert requested(["nts_iv_families.inc"])[ws] >= 2
    assert "hset_q" in C.BY_NAME["hset_sweep"].family & C.BY_NAME["hcount_capped"].family
    for ws, f in C.REQUESTED_TWICE.items():
        assert requested([f])[ws] >= 2, (ws, f)
    users = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".inc", ".hip", ".h")) and "ivs_tmp" in requested([f])]
    assert sum(requested([f])["ivs_tmp"] for f in users) == 29 and len(users) == 8        # (the three edit scripts: two, in nts_edit_fr_script.inc)
    assert C.BY_NAME[C.HEAVY_PARTNER].ivs_tmp and requested(C.SOURCES[C.HEAVY_PARTNER])["ivs_tmp"] == max(requested([f])["ivs_tmp"] for f in users)


def test_neighbours_stay_in_the_dozens_and_leave_no_entry_out():
    pairs = C.neighbours()
    assert len(pairs) == len(set(pairs)) and 24 <= len(pairs) <= 120, len(pairs)
    assert {x for x, _ in pairs} | {y for _, y in pairs} == set(NAMES)
    assert ("edit_script", "edit_wide_script") in pairs and ("edit_wide_script", "edit_script") in pairs
    assert all((n, C.HEAVY_PARTNER) in pairs for n in NAMES if n != C.HEAVY_PARTNER)
    # the calls of every round: both builds in both orders, the engine behind and before a sliced build and before a one-pass build, the
    # FASTA parse with every way of the sketch, the first way into a filter with each of the others, the two filter sweeps
    both = [("graph_build", "graph_build_sliced"), ("graph_build_sliced", "engine_add_blocks"), ("bf_count_intervals", "bf_sample_intervals")]
    both += [("fasta_parse", "sketch_" + w) for w in C.SKETCH_WAYS] + [("bloom_insert", n) for n in ("bloom_insert_and", "bloom_cascade", "bloom_repeats")]
    for x, y in both:
        assert (x, y) in pairs and (y, x) in pairs, (x, y)
    assert ("engine_add_blocks", "graph_build") in pairs
    assert set(C.PAIRED) <= set(pairs)


def functions(files):
    """{name: body} of the functions defined at the left margin of the given sources (a signature may run over several lines; the body
    ends at the first closing brace at the left margin)"""
    out = {}
    for f in files:
        with open(os.path.join(CSRC, f)) as fh:
            lines = fh.read().split("\n")
        i = 0
        while i < len(lines):
            m = re.match(r'^(?:extern "C" )?[A-Za-z_][\w:<>\*&, ]*?\b([A-Za-z_]\w*)\(', lines[i])
            if not m or lines[i].rstrip().endswith(";"):
                i += 1
                continue
            if "{" in lines[i] and lines[i].rstrip().endswith("}"):
                out.setdefault(m.group(1), []).append(lines[i])
                i += 1
                continue
            j = i + 1
            while j < len(lines) and lines[j] != "{" and not lines[j].rstrip().endswith(";") and (lines[j].startswith(" ") or not lines[j]):
                j += 1
            if j >= len(lines) or lines[j] != "{":
                i += 1
                continue
            e = j
            while e < len(lines) and lines[e] != "}":
                e += 1
            out.setdefault(m.group(1), []).append("\n".join(lines[i:e + 1]))
            i = e + 1
    return {name: "\n".join(bodies) for name, bodies in out.items()}


SCRATCH = re.compile(r'\b(?:ws_get|NTS_WS|ws_upload)\(')
ROUND_FILES = ["nts_graph.hip", "nts_fasta_dev.inc", "nts_bf_iv.inc", "nts_bf_sample.inc", "nts_comm.inc"]


def test_every_exported_function_that_requests_scratch_in_the_round_files_is_named():
    """read from the sources: the functions of nts_graph.hip, nts_fasta_dev.inc, nts_bf_iv.inc, nts_bf_sample.inc and nts_comm.inc that
    request scratch (ws_get / NTS_WS / ws_upload), and the library's exported functions (those ntsynt_amd/_lib.py binds) that are one of
    them or reach one through the functions they call, in any source.  Each is called by a catalogue entry (C.CALLS), by the rank test
    (its CALLS), or has an order test of its own"""
    from tests import test_gpu_call_order_ranks as R
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".inc", ".hip", ".h", ".cpp"))]
    every = functions(sources)
    asking = {name for name, body in functions(ROUND_FILES).items() if SCRATCH.search(body.split("\n", 1)[-1])}
    assert {"graph_build_ranges", "slice_bufs", "nts_genome_from_fasta", "nts_mx_kmers", "bf_count_intervals_run", "sample_intervals_run",
            "nts_bf_allreduce_parts", "nts_mx_allgather_ex"} <= asking, sorted(asking)
    code = {name: re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', re.sub(r"//[^\n]*", "", body)) for name, body in every.items()}      # (no comments, no strings)
    calls = {name: {w for w in set(re.findall(r"\b[A-Za-z_]\w*\b", body)) if w in every and w != name} for name, body in code.items()}
    reach = set(asking)
    grew = True
    while grew:
        grew = False
        for name, callees in calls.items():
            if name not in reach and callees & reach:
                reach.add(name)
                grew = True
    with open(os.path.join(os.path.dirname(CSRC), "_lib.py")) as fh:
        exported = set(re.findall(r'\("(nts_\w+)"', fh.read()))
    assert len(exported) > 100
    need = sorted(reach & exported)
    print("exported functions that request scratch in the round files:", need)
    assert {"nts_graph_build", "nts_engine_add", "nts_genome_from_fasta", "nts_bf_count_intervals", "nts_bf_sample_intervals", "nts_mx_kmers",
            "nts_bf_allreduce_and", "nts_bf_allreduce_groups", "nts_bf_allreduce_parts", "nts_mx_allgather", "nts_mx_allgather_ex"} <= set(need), need
    named = {fn: entry for entry, fns in C.CALLS.items() for fn in fns}
    assert set(C.CALLS) <= set(NAMES)
    for fn in need:
        if fn in named:
            continue
        if fn in R.CALLS:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "multirank_worker.py")) as fh:
                assert R.CALLS[fn] in fh.read(), fn
            continue
        assert fn in ELSEWHERE, (fn, "requests scratch in the round files and no entry, rank test or order test names it")
        assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), ELSEWHERE[fn])), fn


# exported functions that reach the round files' scratch and have an order test of their own, outside the catalogue
ELSEWHERE = {}


def test_the_chain_seed_leaves_out_no_entry_and_no_size():
    order = C.chain_order()
    assert len(order) == C.CHAIN_PASSES * len(NAMES)
    assert set(order) == {(n, s) for n in NAMES for s in C.SIZES}
    assert order == C.chain_order() and order != C.chain_order(C.CHAIN_SEED + 1)
    for p in range(C.CHAIN_PASSES):
        assert sorted(n for n, _ in order[p * len(NAMES):(p + 1) * len(NAMES)]) == sorted(NAMES)


# entry -> where its existing test refuses arguments (None: that entry's tests have no such case)
REFUSED_IN = {"edit_segments": "test_gpu_edit_segments.py", "edit_wide": "test_gpu_edit_wide.py", "edit_script": "test_gpu_edit_script.py",
              "edit_wide_script": "test_gpu_edit_wide_script.py", "edit_extend": "test_gpu_edit_extend.py", "edit_extend_script": "test_gpu_edit_extend_script.py",
              "cigar_build": "test_gpu_cigar_build.py", "cigar_lift": "test_gpu_cigar_lift.py", "cigar_lift_stats": "test_gpu_cigar_lift_stats.py",
              "cigar_text": "test_gpu_cigar_text.py", "iv_anchor_segments": "test_gpu_iv_anchor_segments.py",
              "iv_links": None, "iv_sites": "test_gpu_iv_sites.py", "iv_periods": "test_gpu_iv_periods.py", "iv_period_hashes": "test_gpu_iv_period_hashes.py",
              "iv_families": "test_gpu_iv_families.py", "iv_family_sites": "test_gpu_iv_family_sites.py", "hset_sweep": "test_gpu_hset.py",
              "hcount_capped": "test_gpu_hcount.py", "minhash": None, "minhash_intervals": "test_gpu_block_assessment.py", "bloom_insert": None, "engine_add_blocks": None}
REFUSED_IN.update({"sketch_" + w: "test_gpu_sketch_seams.py" for w in C.SKETCH_WAYS})
REFUSED_IN.update({name: None for name in NEW})
# the FASTA parse's own tests refuse a file without a header (tests/test_gpu_fasta.py: the wrapper makes a ValueError of the library's
# NTS_EFORMAT; the entry goes through the C entry point and Context.check).  tests/test_gpu_block_assessment.py refuses a record index
# of minhash_intervals, nothing of minhash_pairs.
REFUSED_IN["fasta_parse"] = "test_gpu_fasta.py"
REFUSED_AS = {"fasta_parse": 'raises(ValueError, match="not a FASTA file")'}          # what the file holds where it is not NtsError


def test_entries_with_a_refused_case_are_the_ones_whose_tests_have_one():
    assert set(REFUSED_IN) == set(NAMES)
    assert {e.name for e in C.ENTRIES if e.refuse} == {n for n, f in REFUSED_IN.items() if f}
    here = os.path.dirname(os.path.abspath(__file__))
    for name, f in REFUSED_IN.items():
        if f:
            with open(os.path.join(here, f)) as fh:
                assert REFUSED_AS.get(name, "NtsError") in fh.read(), (name, f)
    # the calls whose tests refuse nothing: nothing is expected to raise anywhere in the files that test them
    for f in ("test_gpu_bloom_geometry.py", "test_gpu_engine_shapes.py", "test_gpu_interval_edges.py", "test_gpu_fasta_seams.py", "test_gpu_graph_slices.py",
              "test_gpu_stages.py", "test_gpu_configs.py"):
        with open(os.path.join(here, f)) as fh:
            assert "raises(" not in fh.read(), f


def test_expectations_are_plain_bytes_of_the_documented_layouts():
    exp = C.expected_of("iv_periods", "S")
    assert len(exp) == C.case_of("iv_periods", "S")["n_iv"] * 20
    seg = np.frombuffer(C.expected_of("edit_segments", "S"), dtype=np.uint8)
    case = C.case_of("edit_segments", "S")["pair"]
    assert seg.size == len(case.iv_a) * C.IDENTITY.itemsize + 4 * len(case.segs)

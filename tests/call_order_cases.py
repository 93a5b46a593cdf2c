"""The catalogue behind tests/test_gpu_call_order.py (docs/design/04_24_call_order.md): one entry per device entry point that uses the
context's named scratch buffers (ws_get, csrc/nts_internal.h) or its pinned staging area, each with a small input (S) and one at least
four times as large in every dimension that sizes a scratch buffer (L, another seed), the expected result of either from the brute
forces and the oracle alone, and the call itself.  Plain numpy: no GPU, no torch; ntsynt_amd.device is imported inside run() and
refuse() only.  The FASTA entry's expectation is the library's host reader (nts_fasta_read: host code, no device), on a file the case
writes into a directory of the process's own.

What is borrowed from the GPU test modules (imported inside the functions that use them; importing those modules starts nothing):
the input builders (Pair, World, random_lists, array_like, random_occurrences, random_case, random_chains, pairs_of, segment_array,
task_array), which take the record dtypes of ntsynt_amd.device and nothing else from it, and three helpers that are not among the
brute-force modules but only compose them on the CPU: tests.test_gpu_edit_script.expected (identity_brute and variants_brute per
segment), tests.test_gpu_edit_extend_script.expected (extend_brute and variants_brute per task) and
tests.test_gpu_gap_links.brute_links (the link definition over dictionaries; nts_iv_links has no brute-force module of its own).
None of them calls the device.

An entry's `family` is the set of scratch names it requests that some other entry requests too (read from csrc;
tests/test_call_order_cases_host.py holds the table against the sources).  Two entries are neighbours when their families meet.
A result is a `bytes` object: the arrays the call returns one behind the other, so that "equal" means byte for byte."""
import os

import numpy as np

from oracle import nts_oracle as O
from tests import cigar_brute as CB
from tests import cs_brute as CS
from tests import engine_brute as EB
from tests import engine_shapes as ES
from tests import identity_brute as B
from tests import lift_brute as LB
from tests import lift_stats_brute as SB
from tests import wide_brute as W
from tests import wide_variants_brute as WV
from tests.families_brute import as_samples, as_sites, brute_families, brute_family_sites, brute_period_hashes
from tests.helpers import oracle_flat, oracle_set_sample, oracle_sketches, random_records, to_device, to_oracle
from tests.periods_brute import as_array, brute_periods
from tests.sites_brute import brute_sites

SIZES = ("S", "L")
SEED = {"S": 101, "L": 202}                                   # L differs from S in content as well as in size
BAND, MAX_EDITS = 31, 127                                     # the edit family's W and E
PENALTY, EXTEND_EDITS = 6, 255
U64_MAX = (1 << 64) - 1
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)

# the record layouts of include/ntsynt_hip.h, written out here so that expected() needs nothing of ntsynt_amd.device (the host test
# compares them with the device module's)
IDENTITY = np.dtype([(n, "<u8") for n in ("aligned_a", "aligned_b", "edits")] +
                    [(n, "<u4") for n in ("segments", "aligned", "backward", "too_long", "offband", "invalid", "overband", "reserved")])
OP = np.dtype([("seg", "<u4"), ("p", "<u4"), ("q", "<u4"), ("op", "u1"), ("base_a", "u1"), ("base_b", "u1"), ("pad", "u1")])
SEGMENT = np.dtype([("iv_a", "<u4"), ("x", "<u4"), ("dx", "<u4"), ("y_lo", "<u4"), ("dy", "<i4"), ("kind", "<u4")])
EXTEND = np.dtype([(n, "<u4") for n in ("ext_a", "ext_b", "edits", "valid_a", "valid_b")])
CHAIN = np.dtype([(n, "<u8") for n in ("first", "n_cig", "eq", "x", "ins", "del", "len_a", "len_b")])
LIFT_HIT = np.dtype([("pos", "<u8"), ("entry", "<u8"), ("off", "<u8"), ("code", "<u4"), ("reserved", "<u4")])
LIFT_STATS = np.dtype([(n, "<u8") for n in ("oth_lo", "oth_hi", "eq", "x", "src_gap", "oth_gap")] + [("src_gaps", "<u4"), ("oth_gaps", "<u4"), ("reserved", "<u8")])
LINK = np.dtype([(n, "<u4") for n in ("list_a", "iv_a", "list_b", "iv_b", "anchors", "fwd", "rev", "min_off_a", "max_off_a", "min_off_b", "max_off_b")])
SITE = np.dtype([(n, "<u4") for n in ("list_q", "iv_q", "rec_t", "hits", "fwd", "rev", "min_off_q", "max_off_q", "first_t", "last_t")])
SAMPLE = np.dtype([("h0", "<u8"), ("iv", "<u4"), ("off", "<u4")])

# ---- the scratch names that more than one entry point or helper requests (csrc/*.inc, *.hip) ------------------------------------------
EDIT_SHARED = ("edit_seg", "edit_ivs", "edit_dist", "edit_num")
SCRIPT_SHARED = ("edit_first", "edit_kept", "edit_ops", "edit_status", "edit_worst")
CIGX_SHARED = ("cigx_cigar", "cigx_chains", "cigx_prefixes", "cigx_status", "cigx_worst")    # cig_index_stage: the three readers of a round's CIGARs
IVF_SHARED = ("ivf_pair", "ivf_h", "ivf_a", "ivf_h2", "ivf_a2", "ivf_head", "ivf_rid", "ivf_urid", "ivf_num")
BIN_SHARED = ("bin_cnt1", "bin_out1", "bin_cnt2", "bin_out2", "bin_late_ctl", "bin_late")       # the binned Bloom build: insert, insert_and, cascade
# nts_graph_build in one pass and in slices (and nts_engine_add, which runs the same passes): the element columns, the results, the slice buffers
GRAPH_SHARED = ("g_h", "g_asm", "g_rec", "g_pos", "g_keep", "g_list", "g_evid", "g_vhash", "g_orec", "g_opos", "g_cvid", "g_casm", "g_clist", "g_eu", "g_ev",
                "g_ew", "g_ef", "g_srank", "gs_hist", "gs_cnt", "gs_sel_tmp", "gs_h", "gs_idx", "gs_h2", "gs_idx2", "gs_flag", "gs_scan", "gs_valid", "gs_tmp")
# requested more than once inside ONE entry point (another size each time, or fetched again between launches)
REQUESTED_TWICE = {"e_flag": "nts_dgraph.inc", "e_scan": "nts_dgraph.inc", "ivl_tmp": "nts_iv_links.inc", "hset_q": "nts_hcount.inc",
                   "ivs_tmp": "nts_iv_families.inc", "fa_hdr": "nts_fasta_dev.inc", "fa_ctl": "nts_fasta_dev.inc", "gs_idx": "nts_graph.hip",
                   "g_h": "nts_graph.hip", "g_list": "nts_graph.hip"}


def _rows(dtype, tuples):
    out = np.zeros(len(tuples), dtype=dtype)
    for i, t in enumerate(tuples):
        out[i] = tuple(t)
    return out


def _cat(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def dna(rng, n):
    return LETTERS[rng.integers(0, 4, size=n)]


# ======================================================================================================================================
# the edit family: one pair of genomes per size, read by the four segment calls
# ======================================================================================================================================
def make_pair(size, seed):
    """segments of six kinds in turn: a few planted edits, equal strings, so many substitutions that the band is left (and E reaches),
    an indel beyond the band (offband: the wide pass aligns it), an N, an indel beyond E (stays passed).  Strings of at most 300 bases"""
    from tests.test_gpu_edit_segments import Pair, substituted
    from tests.test_gpu_edit_wide import add, inserted
    rng = np.random.default_rng(seed)
    p = Pair(rng)
    n_seg = 36 if size == "S" else 252
    made = 0
    while made < n_seg:
        m = min(int(rng.integers(2, 7)), n_seg - made)
        pairs = []
        for q in range(made, made + m):
            kind = q % 6
            if kind == 0:
                a = dna(rng, int(rng.integers(40, 301)))
                b = list(a)
                for _ in range(int(rng.integers(1, 7))):
                    what, where = int(rng.integers(0, 3)), int(rng.integers(0, len(b)))
                    if what == 0:
                        b[where] = rng.choice(LETTERS[LETTERS != b[where]])
                    elif what == 1 and len(b) > 1:
                        del b[where]
                    else:
                        b.insert(where, rng.choice(LETTERS))
                b = np.array(b, dtype=np.uint8)
            elif kind == 1:
                a = dna(rng, int(rng.integers(1, 200)))
                b = a.copy()
            elif kind == 2:
                a = dna(rng, 300)
                b = substituted(rng, a, np.flatnonzero(rng.random(300) < 0.32))
            elif kind == 3:
                a = dna(rng, int(rng.integers(60, 200)))
                b = inserted(rng, a, int(rng.integers(1, a.size)), int(rng.integers(BAND + 1, 100)))
            elif kind == 4:
                a = dna(rng, int(rng.integers(30, 120)))
                b = a.copy()
                a[int(rng.integers(0, a.size))] = ord("N")
            else:
                a = dna(rng, 60)
                b = inserted(rng, a, 30, MAX_EDITS + 1 + int(rng.integers(0, 100)))
            pairs.append((a, b))
        add(p, pairs, flip=rng.random() < 1 / 3, rec=int(rng.integers(0, 2)), margin=(int(rng.integers(0, 9)), int(rng.integers(0, 9))))
        made += m
    return {"pair": p}


def _pair_host(case):
    "(seq_a, off_a, seq_b, off_b, ivs_a, ivs_b) of the pair as Pair.upload lays the genomes out"
    from tests.test_gpu_edit_script import host_sequences
    p = case["pair"]
    (seq_a, off_a), (seq_b, off_b) = host_sequences(p)
    ivs_a = [(int(off_a[r]) + s, e - s) for r, s, e in p.iv_a]
    ivs_b = [(int(off_b[r]) + s, e - s) for r, s, e in p.iv_b]
    return seq_a, off_a, seq_b, off_b, ivs_a, ivs_b


def _pair_brute(case):
    "the brute forces of the pair, once: narrow, final, per interval (narrow and final), both scripts"
    if "brute" not in case:
        p = case["pair"]
        seq_a, off_a, seq_b, off_b, ivs_a, ivs_b = _pair_host(case)
        dist, per_iv = B.brute_edit(seq_a, seq_b, ivs_a, ivs_b, p.flip, p.segs, BAND)
        narrow, final, per_iv_wide, work = W.brute_wide(seq_a, seq_b, ivs_a, ivs_b, p.flip, p.segs, BAND, MAX_EDITS)
        assert narrow == dist
        from tests.test_gpu_edit_script import expected as script_expected
        _, ops, first, _ = script_expected(p, seq_a, off_a, seq_b, off_b, BAND)
        wops, wfirst, members = WV.expected_ops(seq_a, seq_b, ivs_a, ivs_b, p.flip, p.segs, final, BAND)
        case["brute"] = dict(dist=dist, per_iv=per_iv, final=final, per_iv_wide=per_iv_wide, work=work, ops=ops, first=first, wops=wops,
                             wfirst=wfirst, members=members)
    return case["brute"]


def _identity_bytes(per_iv, results):
    out = np.zeros(len(per_iv), dtype=IDENTITY)
    for i, row in enumerate(per_iv):
        for name, v in row.items():
            out[i][name] = v
    return _cat(out, np.array(results, dtype=np.uint32))


def _ops_bytes(ops, first):
    return _cat(_rows(OP, [o + (0,) for o in ops]), np.array(first, dtype=np.uint64))


def pair_counts(case):
    p, br = case["pair"], _pair_brute(case)
    return {"segments": len(p.segs), "intervals": len(p.iv_a), "ops": len(br["ops"]), "wide_ops": len(br["wops"]), "work_set": len(br["work"]),
            "bases": sum(x.size for r in p.rec_a for x in r)}


def pair_outcomes(case):
    br = _pair_brute(case)
    kinds = [s[5] for s in case["pair"].segs]
    return {"aligned": any(d < B.INVALID for d in br["dist"]), "overband": B.OVERBAND in br["dist"], "invalid": B.INVALID in br["dist"],
            "passed": B.PASSED in br["dist"], "script with an op": len(br["ops"]) > 0,
            "rescued offband": any(kinds[i] == B.OFFBAND and br["final"][i] < B.INVALID for i in br["work"]),
            "rescued overband": any(kinds[i] == B.CANDIDATE and br["final"][i] < B.INVALID for i in br["work"]),
            "still passed": any(k == B.OFFBAND and f == B.PASSED for k, f in zip(kinds, br["final"])),
            "wide member": len(br["members"]) > 0}


def _with_pair(ctx, case, call):
    from tests.test_gpu_edit_wide import segment_array
    p = case["pair"]
    (ga, _, _), (gb, _, _) = p.upload(ctx)
    try:
        return call(ga, gb, p, segment_array(p))
    finally:
        ga.free()
        gb.free()


def run_edit_segments(ctx, case):
    iv, dist = _with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_segments(ga, gb, p.iv_a, p.iv_b, arr, p.flip, BAND, with_distances=True))
    return _cat(iv, dist)


def run_edit_wide(ctx, case):
    narrow = np.array(_pair_brute(case)["dist"], dtype=np.uint32)
    iv, final = _with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, arr, p.flip, BAND, MAX_EDITS, narrow))
    return _cat(iv, final)


def run_edit_script(ctx, case, dist=None):
    dist = np.array(_pair_brute(case)["dist"], dtype=np.uint32) if dist is None else dist
    return _cat(*_with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_script(ga, gb, p.iv_a, p.iv_b, arr, p.flip, BAND, dist)))


def run_edit_wide_script(ctx, case, final=None):
    final = np.array(_pair_brute(case)["final"], dtype=np.uint32) if final is None else final
    return _cat(*_with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_wide_script(ga, gb, p.iv_a, p.iv_b, arr, p.flip, BAND, MAX_EDITS, final)))


def _off_by_one(results, members):
    "the brute force's per-segment results with the first member's distance one too large: refused behind the launch"
    bad = np.array(results, dtype=np.uint32)
    bad[members[0]] += 1
    return bad


def refuse_edit_segments(ctx, case):
    _with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_segments(ga, gb, p.iv_a, p.iv_b, arr, p.flip, 0))


def refuse_edit_wide(ctx, case):
    narrow = np.array(_pair_brute(case)["dist"], dtype=np.uint32)
    _with_pair(ctx, case, lambda ga, gb, p, arr: ctx.edit_wide(ga, gb, p.iv_a, p.iv_b, arr, p.flip, BAND, 62, narrow))


def refuse_edit_script(ctx, case):
    br = _pair_brute(case)
    run_edit_script(ctx, case, _off_by_one(br["dist"], [i for i, d in enumerate(br["dist"]) if 1 <= d < B.INVALID]))


def refuse_edit_wide_script(ctx, case):
    br = _pair_brute(case)
    run_edit_wide_script(ctx, case, _off_by_one(br["final"], br["members"]))


# ---- the free-end extension and its script ------------------------------------------------------------------------------------------
def make_world(size, seed):
    "strings of 50 .. 300 bases with 0 .. 8 % substitutions and an indel now and then; every fourth B turns unrelated half way; mixed flags"
    from tests.test_gpu_edit_extend import World, substituted, unlike
    rng = np.random.default_rng(seed)
    w = World(rng)
    for t in range(24 if size == "S" else 120):
        s = dna(rng, int(rng.integers(50, 301)))
        b = substituted(rng, s, np.flatnonzero(rng.random(s.size) < rng.uniform(0.0, 0.08)))
        while rng.random() < 0.35:
            at, n = int(rng.integers(0, b.size)), int(rng.integers(1, 13))
            b = np.concatenate([b[:at], dna(rng, n), b[at:]]) if rng.random() < 0.5 else np.delete(b, slice(at, at + n))
        if t % 4 == 3:
            b = np.concatenate([b[:b.size // 2], unlike(rng, s[b.size // 2:])])
        if b.size == 0 or b.size > 300:
            b = s.copy()
        w.place(s, b, flags=int(rng.integers(0, 8)), rec=int(rng.integers(0, 2)))
    return {"world": w}


def _world_brute(case):
    if "brute" not in case:
        from tests.test_gpu_edit_extend_script import expected as extend_expected
        case["brute"] = extend_expected(case["world"], PENALTY, EXTEND_EDITS)
    return case["brute"]


def world_counts(case):
    exp = _world_brute(case)
    return {"tasks": len(exp), "ops": sum(len(e[1]) for e in exp), "bases": sum(x.size for r in case["world"].rec_a for x in r)}


def world_outcomes(case):
    exp = _world_brute(case)
    return {"reaches an end": any(e[0][0] == e[0][3] or e[0][1] == e[0][4] for e in exp),
            "stops early": any(e[0][0] < e[0][3] and e[0][1] < e[0][4] for e in exp),
            "with edits": any(e[0][2] > 0 for e in exp), "without an edit": any(e[0][2] == 0 for e in exp)}


def expected_edit_extend(case):
    return _cat(_rows(EXTEND, [e[0] for e in _world_brute(case)]))


def expected_edit_extend_script(case):
    exp = _world_brute(case)
    return _ops_bytes([op for e in exp for op in e[1]], np.concatenate([[0], np.cumsum([len(e[1]) for e in exp])]))


def _with_world(ctx, case, call):
    from tests.test_gpu_edit_extend import task_array
    ga, gb = case["world"].upload(ctx)
    try:
        return call(ga, gb, task_array(case["world"].tasks))
    finally:
        ga.free()
        gb.free()


def run_edit_extend(ctx, case):
    return _cat(_with_world(ctx, case, lambda ga, gb, tasks: ctx.edit_extend(ga, gb, tasks, PENALTY, EXTEND_EDITS)))


def run_edit_extend_script(ctx, case, results=None):
    results = _rows(EXTEND, [e[0] for e in _world_brute(case)]) if results is None else results
    return _cat(*_with_world(ctx, case, lambda ga, gb, tasks: ctx.edit_extend_script(ga, gb, tasks, results)))


def refuse_edit_extend(ctx, case):
    def call(ga, gb, tasks):
        tasks["flags"][1] = 8
        ctx.edit_extend(ga, gb, tasks, PENALTY, EXTEND_EDITS)
    _with_world(ctx, case, call)


def refuse_edit_extend_script(ctx, case):
    "a task's edits one too many: found by the kernel"
    results = _rows(EXTEND, [e[0] for e in _world_brute(case)])
    at = int(np.flatnonzero(results["edits"] > 0)[0])
    results["edits"][at] += 1
    run_edit_extend_script(ctx, case, results)


# ======================================================================================================================================
# CIGARs
# ======================================================================================================================================
def make_cigar(size, seed):
    from tests.test_gpu_cigar_build import random_case
    n_pieces, n_chains = (40, 6) if size == "S" else (200, 30)
    pieces, scripts = random_case(seed, n_pieces, n_chains)
    ops = [(t, p, q, op, 0xFF, 0xFF, 0) for t, s in enumerate(scripts) for op, p, q in s]
    return {"pieces": pieces, "ops": ops, "first": np.concatenate([[0], np.cumsum([len(s) for s in scripts])]).astype(np.uint64), "n_chains": n_chains}


def cigar_counts(case):
    entries, _ = CB.brute_cigar(case["pieces"], case["ops"], case["first"], case["n_chains"])
    return {"pieces": len(case["pieces"]), "ops": len(case["ops"]), "chains": case["n_chains"], "entries": len(entries)}


def cigar_outcomes(case):
    entries, chains = CB.brute_cigar(case["pieces"], case["ops"], case["first"], case["n_chains"])
    return {"every kind of entry": {e & 15 for e in entries} == set(CB.CODE.values()), "a reversed piece": any(p[3] for p in case["pieces"]),
            "a chain of several entries": any(c["n_cig"] > 1 for c in chains)}


def expected_cigar_build(case):
    entries, chains = CB.brute_cigar(case["pieces"], case["ops"], case["first"], case["n_chains"])
    return _cat(np.array(entries, dtype=np.uint64), _rows(CHAIN, [tuple(c[f] for f in CHAIN.names) for c in chains]))


def _cigar_arrays(case):
    from ntsynt_amd.device import OP_DTYPE, PIECE_DTYPE
    return _rows(PIECE_DTYPE, case["pieces"]), _rows(OP_DTYPE, case["ops"]), case["first"]


def run_cigar_build(ctx, case):
    pc, ops, first = _cigar_arrays(case)
    return _cat(*ctx.cigar_build(pc, ops, first, case["n_chains"]))


def refuse_cigar_build(ctx, case):
    "a piece one base longer than its script makes it: found by the kernel"
    pc, ops, first = _cigar_arrays(case)
    pc["n"][int(np.flatnonzero(np.diff(first.astype(np.int64)) > 0)[0])] += 1
    ctx.cigar_build(pc, ops, first, case["n_chains"])


def make_lift(size, seed):
    from tests.test_gpu_cigar_lift import random_chains
    n_chains, n_entries, n_queries = (6, 30, 48) if size == "S" else (30, 150, 240)
    lists = random_chains(seed, n_chains, n_entries)
    rng = np.random.default_rng(seed + 1)
    chains, at = [], 0
    for entries in lists:
        count = {code: sum(v >> 4 for v in entries if v & 15 == code) for code in CB.CODE.values()}
        eq, x, ins, dele = count[7], count[8], count[1], count[2]
        chains.append((at, len(entries), eq, x, ins, dele, eq + x + dele, eq + x + ins))
        at += len(entries)
    queries = []
    for _ in range(n_queries):
        c, side = int(rng.integers(0, n_chains)), int(rng.integers(0, 2))
        queries.append((c, side, int(rng.integers(0, chains[c][7 if side else 6] + 1))))
    queries[-1] = (n_chains - 1, 0, chains[-1][6])           # the end of the last chain
    # cigar_lift_stats: as many random valid ranges, every fourth at most seven bases long (rng of its own: the queries stay as they were)
    rng = np.random.default_rng(seed + 2)
    ranges = []
    while len(ranges) < n_queries:
        c, side = int(rng.integers(0, n_chains)), int(rng.integers(0, 2))
        n = chains[c][7 if side else 6]
        lo, hi = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        if lo < hi:
            ranges.append((c, side, lo, hi if len(ranges) % 4 else min(lo + int(rng.integers(1, 8)), n)))
    # cigar_text: two genomes of one record each, the chains one behind the other on both with a few bases between them; every third
    # chain lies backwards on b, where its span names the last of its bases
    rng = np.random.default_rng(seed + 3)
    spans, at_a, at_b = [], int(rng.integers(0, 5)), int(rng.integers(0, 5))
    for c, ch in enumerate(chains):
        back = c % 3 == 1
        spans.append((at_a, at_b + ch[7] - 1 if back and ch[7] else at_b, 0, 0, 1 if back else 0, 0))
        at_a, at_b = at_a + ch[6] + int(rng.integers(0, 5)), at_b + ch[7] + int(rng.integers(0, 5))
    return {"lists": lists, "chains": chains, "queries": queries, "ranges": ranges, "spans": spans, "seq_a": dna(rng, at_a), "seq_b": dna(rng, at_b)}


def _lift_hits(case):
    walkers = {}
    out = []
    for c, side, pos in case["queries"]:
        if c not in walkers:
            walkers[c] = LB.Walker(case["lists"][c], case["chains"][c][0])
        out.append(walkers[c].lift(side, pos))
    return out


def lift_counts(case):
    return {"entries": sum(len(x) for x in case["lists"]), "chains": len(case["chains"]), "queries": len(case["queries"])}


def lift_outcomes(case):
    "a hit: the position is an aligned base; a miss: it lies in a gap of the other side, or is the chain's end"
    codes = [h[3] for h in _lift_hits(case)]
    return {"hit": any(c in (7, 8) for c in codes), "miss in a gap": any(c in (1, 2) for c in codes), "the end of a chain": 0 in codes}


def expected_cigar_lift(case):
    return _cat(_rows(LIFT_HIT, [h + (0,) for h in _lift_hits(case)]))


def _lift_arrays(case):
    from ntsynt_amd.device import CHAIN_DTYPE, LIFT_QUERY_DTYPE
    return np.array([v for x in case["lists"] for v in x], dtype=np.uint64), _rows(CHAIN_DTYPE, case["chains"]), _rows(LIFT_QUERY_DTYPE, case["queries"])


def run_cigar_lift(ctx, case):
    return _cat(ctx.cigar_lift(*_lift_arrays(case)))


def refuse_cigar_lift(ctx, case):
    "a query beyond its chain's end: found by the kernel"
    cigar, chains, queries = _lift_arrays(case)
    queries["pos"][len(queries) // 2] = int(chains[int(queries["chain"][len(queries) // 2])]["len_a"]) + int(chains["len_b"].max()) + 1
    ctx.cigar_lift(cigar, chains, queries)


def _lift_stats(case):
    if "stats" not in case:
        counters = [SB.Counter(entries) for entries in case["lists"]]
        case["stats"] = [counters[c].stats(side, lo, hi) for c, side, lo, hi in case["ranges"]]
    return case["stats"]


def lift_stats_counts(case):
    return {"entries": sum(len(x) for x in case["lists"]), "chains": len(case["chains"]), "ranges": len(case["ranges"])}


def lift_stats_outcomes(case):
    stats = [dict(zip(SB.FIELDS, s)) for s in _lift_stats(case)]
    return {"a mismatch": any(s["x"] for s in stats), "a gap of the source": any(s["src_gap"] for s in stats), "a gap of the other side": any(s["oth_gap"] for s in stats),
            "two runs of one gap kind": any(s["src_gaps"] > 1 for s in stats), "a range inside one entry": any(s["eq"] + s["x"] + s["src_gap"] + s["oth_gap"] == 1 for s in stats)}


def expected_cigar_lift_stats(case):
    return _cat(_rows(LIFT_STATS, [s + (0,) for s in _lift_stats(case)]))


def _lift_ranges(case):
    from ntsynt_amd.device import LIFT_RANGE_DTYPE
    return _lift_arrays(case)[:2] + (_rows(LIFT_RANGE_DTYPE, case["ranges"]),)


def run_cigar_lift_stats(ctx, case):
    return _cat(ctx.cigar_lift_stats(*_lift_ranges(case)))


def refuse_cigar_lift_stats(ctx, case):
    "a range beyond its chain's end: found by the kernel"
    cigar, chains, ranges = _lift_ranges(case)
    at = len(ranges) // 2
    ranges["hi"][at] = int(chains[int(ranges["chain"][at])]["len_b" if ranges["side"][at] else "len_a"]) + 1
    ctx.cigar_lift_stats(cigar, chains, ranges)


def _lift_texts(case):
    "(cg texts, cs texts) per chain, from the entries and the two genomes alone"
    if "texts" not in case:
        cg, cs = [], []
        for entries, ch, sp in zip(case["lists"], case["chains"], case["spans"]):
            start_b = sp[1] - (ch[7] - 1) if sp[4] and ch[7] else sp[1]
            target, query = case["seq_a"][sp[0]:sp[0] + ch[6]], case["seq_b"][start_b:start_b + ch[7]]
            cg.append(CS.cg_from_cigar(entries))
            cs.append(CS.cs_from_cigar(entries, target, CS.reverse_complement(query) if sp[4] else query))
        case["texts"] = cg, cs
    return case["texts"]


def lift_text_counts(case):
    cg, cs = _lift_texts(case)
    return {"entries": sum(len(x) for x in case["lists"]), "chains": len(case["chains"]), "cg_bytes": sum(map(len, cg)), "cs_bytes": sum(map(len, cs))}


def lift_text_outcomes(case):
    cs = _lift_texts(case)[1]
    return {"a forward chain": any(not sp[4] for sp in case["spans"]), "a backward chain": any(sp[4] for sp in case["spans"]),
            "every kind of token": all(any(sign in t for t in cs) for sign in ":*-+"), "every base": all(any(b in t for t in cs) for b in "acgt")}


def expected_cigar_text(case):
    out = []
    for texts in _lift_texts(case):
        out += [np.frombuffer("".join(texts).encode(), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)]
    return _cat(*out)


def run_cigar_text(ctx, case, cigar=None):
    "both texts, with spans; the two genomes are uploaded here and freed again.  cigar: entries other than the case's (the refused ones)"
    from ntsynt_amd.device import CIG_SPAN_DTYPE, Genome
    entries, chains, _ = _lift_arrays(case)
    genomes = []
    try:
        for seq in (case["seq_a"], case["seq_b"]):
            genomes.append(Genome(ctx, ["r"], seq, np.zeros(1, dtype=np.uint64), np.array([seq.size], dtype=np.uint64)))
        return _cat(*ctx.cigar_text(entries if cigar is None else cigar, chains, _rows(CIG_SPAN_DTYPE, case["spans"]), *genomes))
    finally:
        for g in genomes:
            g.free()


def refuse_cigar_text(ctx, case):
    "an entry of length 0: found behind the scan"
    cigar = _lift_arrays(case)[0]
    cigar[cigar.size // 2] &= np.uint64(15)
    run_cigar_text(ctx, case, cigar)


# ======================================================================================================================================
# the interval calls: lists of sampled records in, joins out
# ======================================================================================================================================
def _triples(rec):
    return list(zip(rec["h0"].tolist(), rec["iv"].tolist(), rec["off"].tolist()))


def make_anchor_segments(size, seed):
    from tests.test_gpu_iv_anchor_segments import K, random_lists, records
    n_each, n_pairs = (60, 3) if size == "S" else (300, 15)
    a, b, mate, len_b, flip = random_lists(np.random.default_rng(seed), n_each, n_pairs)
    return {"a": a, "b": b[:n_each], "ra": records(a), "rb": records(b[:n_each]), "mate": mate, "len_b": len_b, "flip": flip, "k": K}


def _anchor_brute(case):
    return B.brute_segments(case["a"], case["b"], case["mate"], case["len_b"], case["flip"], case["k"], BAND, 4096)


def expected_anchor_segments(case):
    segs, per_iv = _anchor_brute(case)
    return _cat(_rows(SEGMENT, segs), np.array(per_iv, dtype=np.uint32))


def run_anchor_segments(ctx, case, band=BAND):
    return _cat(*ctx.iv_anchor_segments(case["ra"], case["rb"], case["mate"], case["len_b"], case["flip"], case["k"], band, 4096))


def make_links(size, seed):
    "three lists over gaps that draw from one pool of hashes per group: links of several anchors, and hashes a list holds twice"
    rng = np.random.default_rng(seed)
    n_groups, per_gap = (4, 12) if size == "S" else (20, 15)
    lists = []
    for _ in range(3):
        perm = rng.permutation(n_groups)
        ids = (np.arange(n_groups)[:, None] * 40 + rng.integers(0, 40, size=(n_groups, per_gap))).ravel()
        h = (ids.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        iv, off = np.repeat(perm, per_gap), rng.integers(0, 5000, size=ids.size)
        order = rng.permutation(ids.size)
        lists.append([(int(x), int(y), int(z)) for x, y, z in zip(h[order], iv[order], off[order])])
    return {"lists": lists, "min_anchors": 2}


def _links_brute(case, min_anchors=None):
    from tests.test_gpu_gap_links import brute_links          # (the definitions over dictionaries; no device call in it)
    return brute_links(case["lists"], case["min_anchors"] if min_anchors is None else min_anchors)


def run_links(ctx, case):
    arrs = [_rows(SAMPLE, lst) for lst in case["lists"]]
    return _cat(ctx.iv_links(arrs, case["min_anchors"]))


def make_sites(size, seed):
    "two lists of gaps against one target, hashes from a small pool: multiplicity on both sides, sites of one pair and of several"
    rng = np.random.default_rng(seed)
    n_q, n_gaps, n_t, n_pool = (30, 3, 60, 25) if size == "S" else (150, 15, 300, 125)
    pool = rng.integers(0, 1 << 62, size=n_pool, dtype=np.uint64)
    lists = []
    for _ in range(2):
        part = np.zeros(n_q, dtype=SAMPLE)
        part["h0"], part["iv"], part["off"] = pool[rng.integers(0, n_pool, size=n_q)], np.sort(rng.integers(0, n_gaps, size=n_q)), rng.integers(0, 6000, size=n_q)
        lists.append(part)
    tgt = np.zeros(n_t, dtype=SAMPLE)
    tgt["h0"], tgt["iv"], tgt["off"] = pool[rng.integers(0, n_pool, size=n_t)], rng.integers(0, 3, size=n_t), rng.integers(0, 40 * n_t, size=n_t)
    return {"lists": lists, "target": tgt, "step": 60, "min_hits": 2}


def run_sites(ctx, case, min_hits=None):
    return _cat(ctx.iv_sites(case["lists"], case["target"], case["step"], case["min_hits"] if min_hits is None else min_hits))


def make_periods(size, seed):
    from tests.test_gpu_iv_periods import array_like
    n, n_iv = (60, 3) if size == "S" else (300, 15)
    return {"rec": array_like(np.random.default_rng(seed), n, n_iv), "n_iv": n_iv}


def expected_periods(case):
    return _cat(as_array(brute_periods(_triples(case["rec"]), case["n_iv"])))


def make_period_hashes(size, seed):
    from tests.test_gpu_iv_period_hashes import array_like
    n, n_iv = (60, 3) if size == "S" else (300, 15)
    rec, periods = array_like(np.random.default_rng(seed), n, n_iv)
    return {"rec": rec, "n_iv": n_iv, "period": periods}


def expected_period_hashes(case):
    return _cat(as_samples(brute_period_hashes(_triples(case["rec"]), case["n_iv"], case["period"])))


def _beyond(case):
    "the records with the last one's interval at n_iv: refused"
    rec = case["rec"].copy()
    rec["iv"][-1] = case["n_iv"]
    return rec


def make_families(size, seed):
    "arrays in groups of four, each group with a pool of hashes of its own; now and then a hash of the next group's pool"
    rng = np.random.default_rng(seed)
    n, n_arrays = (48, 12) if size == "S" else (240, 60)
    a = rng.integers(0, n_arrays, size=n)
    a[a == 5] = 6                                             # an array without a pair
    pools = rng.integers(0, U64_MAX, size=(n_arrays // 4, 6), dtype=np.uint64, endpoint=True)
    g = a // 4
    bridge = (rng.random(n) < 0.04) & (g % 3 == 0) & (g + 1 < n_arrays // 4)
    h = pools[np.where(bridge, g + 1, g), rng.integers(0, 6, size=n)]
    return {"pairs": list(zip(h.tolist(), a.tolist())), "n_arrays": n_arrays}


def expected_families(case):
    family, hashes, hash_family = brute_families(case["pairs"], case["n_arrays"])
    return _cat(np.array(family, dtype=np.uint32), np.array(hashes, dtype=np.uint64), np.array(hash_family, dtype=np.uint32))


def run_families(ctx, case, n_arrays=None):
    from tests.test_gpu_iv_families import pairs_of
    return _cat(*ctx.iv_families(pairs_of(case["pairs"]), case["n_arrays"] if n_arrays is None else n_arrays))


def make_family_sites(size, seed):
    from tests.test_gpu_iv_family_sites import random_occurrences
    n, n_rec, n_fam = (60, 2, 3) if size == "S" else (300, 8, 12)
    occ, family_of = random_occurrences(np.random.default_rng(seed), n, n_rec, n_fam, 20 * n // n_rec)
    return {"occ": occ, "family_of": family_of, "step": 150, "min_hits": 2}


def _family_sites_brute(case, min_hits=None):
    return brute_family_sites(_triples(case["occ"]), case["family_of"], case["step"], case["min_hits"] if min_hits is None else min_hits)


def run_family_sites(ctx, case, min_hits=None):
    hashes = np.array(sorted(case["family_of"]), dtype=np.uint64)
    hash_family = np.array([case["family_of"][h] for h in sorted(case["family_of"])], dtype=np.uint32)
    return _cat(ctx.iv_family_sites(case["occ"], hashes, hash_family, case["step"], case["min_hits"] if min_hits is None else min_hits))


# ======================================================================================================================================
# genomes: the exact set and its counter, MinHash, the sketch on each of its ways, the Bloom build
# ======================================================================================================================================
def _genome(size, seed, bp_s, bp_l, n_frac=0.003):
    rng = np.random.default_rng(seed)
    total = bp_s if size == "S" else bp_l
    lengths = [total // 2, total // 3, total - total // 2 - total // 3]
    seqs = random_records(rng, lengths, n_frac=n_frac)
    return rng, [f"c{i}" for i in range(len(seqs))], seqs


def _mutated(rng, seqs, rate):
    out = []
    for s in seqs:
        a = np.frombuffer(s, dtype=np.uint8).copy()
        hit = (rng.random(a.size) < rate) & (a != ord("N"))
        a[hit] = LETTERS[rng.integers(0, 4, size=int(hit.sum()))]
        out.append(a.tobytes())
    return out


def make_set_sweep(size, seed):
    "a genome of 6 / 30 kbp, the hashes of a mutated copy as the set, membership queries, overlapping intervals over all records"
    k = 24
    rng, names, seqs = _genome(size, seed, 6_000, 30_000)
    n_iv = 6 if size == "S" else 36
    iv = []
    for i in range(n_iv):
        rec = i % len(seqs)
        start = int(rng.integers(0, len(seqs[rec]) - 400))
        iv.append((rec, start, start + int(rng.integers(200, 1200))))
    per_rec = [(p.astype(np.int64), h) for p, h in (O.hash_all(s, k) for s in seqs)]
    members = np.concatenate([O.hash_all(s, k)[1] for s in _mutated(rng, seqs, 0.02)])
    queries = np.concatenate([members[::5], np.concatenate([h for _, h in per_rec])[::7]])      # members and k-mers of the genome, in the set or not
    return {"names": names, "seqs": seqs, "k": k, "iv": iv, "per_rec": per_rec, "members": members, "queries": queries, "rate": 1, "cap": 1}


def _set_sample(case):
    return oracle_set_sample(case["per_rec"], case["seqs"], case["k"], case["members"], case["iv"], case["rate"])


def set_counts(case):
    recs, _ = _set_sample(case)
    return {"intervals": len(case["iv"]), "members": int(case["members"].size), "records": int(recs.size), "bases": sum(len(s) for s in case["seqs"])}


def expected_set_sweep(case):
    return _cat(np.isin(case["queries"], case["members"]).astype(np.uint8), *_set_sample(case))


def run_set_sweep(ctx, case, iv=None):
    from ntsynt_amd.device import HashSet
    g = to_device(ctx, case["names"], case["seqs"])
    hs = None
    try:
        hs = HashSet(ctx, case["members"])
        held = hs.contains(case["queries"]).astype(np.uint8)
        return _cat(held, *g.hset_sample_intervals(hs, case["iv"] if iv is None else iv, case["k"], case["rate"]))
    finally:
        if hs is not None:
            hs.free()
        g.free()


def _count_brute(case):
    "(hits per interval, the count of every member asked for, the capped records, their number per interval)"
    recs, per_iv = _set_sample(case)
    keys, inverse, mult = np.unique(recs["h0"], return_inverse=True, return_counts=True)
    asked = case["members"][::3]
    count_of = dict(zip(keys.tolist(), mult.tolist()))
    read = np.array([count_of.get(int(h), 0) for h in asked], dtype=np.uint32)
    kept = recs[mult[inverse] <= case["cap"]]
    return per_iv, read, kept, np.bincount(kept["iv"].astype(np.int64), minlength=len(case["iv"])).astype(np.uint64)


def expected_count_table(case):
    return _cat(*_count_brute(case))


def run_count_table(ctx, case, iv=None):
    "the set, its counter filled by the count sweep, the counts read back by key, the capped sample"
    from ntsynt_amd.device import HashCounts, HashSet
    g = to_device(ctx, case["names"], case["seqs"])
    hs = hc = None
    try:
        hs = HashSet(ctx, case["members"])
        hc = HashCounts(ctx, hs)
        hits = g.hset_count_intervals(hs, hc, case["iv"] if iv is None else iv, case["k"], case["rate"])
        read = hc.read(case["members"][::3])
        kept, per_iv = g.hset_sample_intervals_capped(hs, hc, case["cap"], case["iv"], case["k"], case["rate"])
        return _cat(hits, read, kept, per_iv)
    finally:
        if hc is not None:
            hc.free()
        if hs is not None:
            hs.free()
        g.free()


def _bad_record(case):
    return case["iv"][:1] + [(len(case["seqs"]), 0, 100)]


def make_minhash(size, seed):
    k = 24
    rng, names, seqs = _genome(size, seed, 5_000, 25_000)
    n_iv, s = (6, 32) if size == "S" else (30, 128)
    iv = []
    for i in range(n_iv):
        rec = i % len(seqs)
        start = int(rng.integers(0, len(seqs[rec]) - 600))
        iv.append((rec, start, start + int(rng.integers(300, 1500))))
    return {"names": names, "seqs": seqs, "k": k, "s": s, "iv": iv}


def expected_minhash(case):
    h = np.unique(np.concatenate([O.hash_all(x, case["k"])[1] for x in case["seqs"]]))
    return _cat(h[h != np.uint64(U64_MAX)][:case["s"]])


def run_minhash(ctx, case):
    g = to_device(ctx, case["names"], case["seqs"])
    try:
        return _cat(g.minhash(case["k"], case["s"]))
    finally:
        g.free()


def expected_minhash_intervals(case):
    sk, nk = oracle_sketches(case["seqs"], case["k"], case["s"], case["iv"])
    out = np.zeros((len(sk), case["s"]), dtype=np.uint64)
    for i, h in enumerate(sk):
        out[i, :h.size] = h
    return _cat(out, np.array([h.size for h in sk], dtype=np.uint32), np.array(nk, dtype=np.uint64))


def run_minhash_intervals(ctx, case, iv=None):
    g = to_device(ctx, case["names"], case["seqs"])
    try:
        return _cat(*g.minhash_intervals(case["iv"] if iv is None else iv, case["k"], case["s"]))
    finally:
        g.free()


# the ways of the sketch that a context can be told to take (tests/test_gpu_sketch_seams.py forces the same): name -> (w, filter, setup)
SKETCH_WAYS = {
    "dense": (64, "relative", lambda c: c.sketch_mode("dense")),
    "pruned_hi": (300, "relative", lambda c: (c.sketch_mode("pruned"), c.sketch_select("hi"))),
    "pruned_full": (300, "relative", lambda c: (c.sketch_mode("pruned"), c.sketch_select("full"))),
    "tiers": (250, "relative", lambda c: c.sketch_tiers("always")),
    "accept_list": (100, "sparse", lambda c: c.sketch_summary("auto")),
}


# what the counters of the last call say of the way it went (as tests/test_gpu_sketch_seams.py reads them), and the last call's counters
# per (way, bases of the genome)
SKETCH_CHECK = {"dense": lambda st: st["candidates"] == 0 and st["tiers"] == 0, "pruned_hi": lambda st: st["candidates"] > 0 and st["tiers"] == 0,
                "pruned_full": lambda st: st["candidates"] > 0 and st["tiers"] == 0, "tiers": lambda st: st["tiers"] >= 2,
                "accept_list": lambda st: st["summary_shift"] >= 7 and st["tiers"] == 0}
SKETCH_WENT = {}
WINDOW_LIMIT = 12000                                          # the largest window (WIN_MAX_W, csrc/nts_internal.h): one more is refused


def make_sketch(way):
    def make(size, seed):
        "a genome of 16 / 80 kbp; the filter: the oracle's of a relative 3 % away, or one k-mer in sixteen of the genome's own"
        k = 24
        w, kind, _ = SKETCH_WAYS[way]
        rng, names, seqs = _genome(size, seed, 16_000, 80_000)
        og = to_oracle(names, seqs)
        nbytes = O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.04))
        if kind == "relative":
            bf = O.bf_build(to_oracle(names, _mutated(rng, seqs, 0.03)), k, nbytes)
        else:
            h0 = np.concatenate([O.hash_all(s, k)[1] for s in seqs])
            bits = np.zeros(nbytes * 8, dtype=bool)
            bits[(h0[(h0 >> np.uint64(40)) % np.uint64(16) == 0] % np.uint64(nbytes * 8)).astype(np.int64)] = True
            bf = np.packbits(bits, bitorder="little")
        return {"names": names, "seqs": seqs, "og": og, "k": k, "w": w, "bf": bf, "way": way}
    return make


def _sketch_brute(case):
    return oracle_flat(O.minimize(case["og"], case["k"], case["w"], case["bf"]))


def sketch_counts(case):
    return {"bases": case["og"].total_bp, "minimizers": int(_sketch_brute(case)[0].size), "filter_bytes": int(case["bf"].size)}


def expected_sketch(case):
    h1, rec, pos = _sketch_brute(case)
    return _cat(h1.astype(np.uint64), rec.astype(np.uint32), pos.astype(np.uint64))


def run_sketch(ctx, case, w=None):
    "w: a window other than the case's (the refused one, beyond the window limit)"
    from ntsynt_amd.device import BloomFilter, sketch
    g = to_device(ctx, case["names"], case["seqs"])
    bf = mx = None
    try:
        bf = BloomFilter(ctx, case["bf"].size, case["k"])
        bf.from_numpy(case["bf"])
        SKETCH_WAYS[case["way"]][2](ctx)
        mx = sketch(ctx, g, case["k"], case["w"] if w is None else w, bf)
        out = _cat(*mx.to_numpy())
        SKETCH_WENT[(case["way"], case["og"].total_bp)] = {"candidates": ctx.sketch_stats()[0], "tiers": ctx.sketch_tiers()[2], "summary_shift": ctx.sketch_summary()}
        return out
    finally:
        ctx.sketch_mode("auto", 0)
        ctx.sketch_select("auto")
        ctx.sketch_tiers("auto")
        ctx.sketch_summary("auto")
        for x in (mx, bf, g):
            if x is not None:
                x.free()


def make_bloom(size, seed):
    k = 24
    _, names, seqs = _genome(size, seed, 16_000, 80_000)
    og = to_oracle(names, seqs)
    return {"names": names, "seqs": seqs, "og": og, "k": k, "nbytes": O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.025))}


def expected_bloom(case):
    return _cat(O.bf_build(case["og"], case["k"], case["nbytes"]))


def run_bloom(ctx, case):
    from ntsynt_amd.device import BloomFilter
    g = to_device(ctx, case["names"], case["seqs"])
    bf = None
    try:
        bf = BloomFilter(ctx, case["nbytes"], case["k"])
        bf.insert(g)
        return _cat(bf.to_numpy())
    finally:
        if bf is not None:
            bf.free()
        g.free()


# ---- the device graph engine: `add` followed by `blocks` on the shapes of tests/engine_shapes.py's "paths" case ------------------------
def make_engine(size, seed):
    lay = EB.Layout(3, seed=seed)
    scale = 1 if size == "S" else 4
    for n in (3, 4) * scale:
        lay.ring(n)
    for _ in range(scale):
        lay.fork((1, 1, 5))
        lay.isolated()
    for i, n in enumerate((2, 3, 10, 17) * scale):
        lay.chain(n * scale, reverse_in=(2,) if i % 2 else ())
    return {"G": 3, "par": dict(bp=ES.BIG, n=1), "script": ES.FIRST(lay.lists)}


def _canonical(trace):
    "a trace of ES.play as text: sets and dictionaries in sorted order"
    def fix(x):
        if isinstance(x, dict):
            return sorted((repr(fix(k)), fix(v)) for k, v in x.items())
        if isinstance(x, (set, frozenset)):
            return sorted(fix(v) for v in x)
        if isinstance(x, (list, tuple)):
            return [fix(v) for v in x]
        return int(x) if isinstance(x, (np.integer, bool)) else x
    return repr([(name, fix(res), fix(graph)) for name, res, graph in trace]).encode()


def engine_counts(case):
    trace, _ = ES.oracle_trace(case)
    return {"records": sum(len(x) for x in case["script"][0][1]), "minimizers": sum(len(r) for x in case["script"][0][1] for r in x),
            "vertices": len(trace[0][2][0]), "edges": len(trace[0][2][1]), "paths": len(trace[-1][1]["paths"])}


def expected_engine(case):
    return _canonical(ES.oracle_trace(case)[0])


def run_engine(ctx, case):
    dev = ES.Dev(ctx, case["G"], **case["par"])
    try:
        return _canonical(ES.play(dev, case["script"]))
    finally:
        dev.free()


# ======================================================================================================================================
# the calls of every round: the FASTA parse, the graph build in one pass and in slices, the other ways into a filter, the filter sweeps
# over intervals, the screen of a minimizer list and the pair counts of MinHash sketches
# ======================================================================================================================================
_tmp_dir = []


def _tmp_path(name):
    "a file of this process's own, in a directory that goes with the process"
    import atexit
    import shutil
    import tempfile
    if not _tmp_dir:
        _tmp_dir.append(tempfile.mkdtemp(prefix="call_order_"))
        atexit.register(shutil.rmtree, _tmp_dir[0], ignore_errors=True)
    return os.path.join(_tmp_dir[0], name)


def make_fasta(size, seed):
    """a file of 24 / 1100 records in lines of 60 and 61 bases: headers with and without a description, lower-case runs, N runs, records
    of length 0, a CRLF record now and then, the last line without a line feed.  At L the headers outnumber the first attempt's table of
    1024 (nts_genome_from_fasta asks for "fa_hdr" a second time, larger) and the file has several tiles"""
    rng = np.random.default_rng(seed)
    n_rec = 24 if size == "S" else 1100
    out = bytearray()
    for r in range(n_rec):
        eol = b"\r\n" if r % 7 == 3 else b"\n"
        out += b">r%d" % r + (b" record %d of the case\tand a tab" % r if r % 3 else b"") + eol
        if r % 5 == 2:
            continue                                          # a record of length 0
        n = int(rng.integers(1, 700)) if (size == "S" or r % 100 == 0) else int(rng.integers(1, 120))
        seq = dna(rng, n)
        if r % 4 == 1 and n > 10:
            a = int(rng.integers(0, n - 5))
            seq[a:a + int(rng.integers(1, 40))] |= 0x20        # a lower-case run
        if r % 6 == 4 and n > 10:
            a = int(rng.integers(0, n - 5))
            seq[a:a + int(rng.integers(1, 30))] = ord("N")
        width = 60 + r % 2
        for at in range(0, n, width):
            out += seq[at:at + width].tobytes() + eol
    while out[-1:] in (b"\n", b"\r"):
        del out[-1:]                                          # the last line ends with the file
    path = _tmp_path(f"fasta_{size}.fa")
    with open(path, "wb") as fh:
        fh.write(bytes(out))
    return {"path": path, "raw": bytes(out)}


def _fasta_host(case):
    "the host reader's records of the case's file (nts_fasta_read: no device code)"
    if "host" not in case:
        from ntsynt_amd import fasta as fa
        case["host"] = fa.read_fasta(case["path"])
    return case["host"]


def _fasta_bytes(recs, bases):
    names = "\0".join(recs.names).encode()
    fai = np.array([row[2:] for row in recs.fai_rows], dtype=np.uint64).reshape(-1, 3)
    return _cat(np.frombuffer(names, dtype=np.uint8), np.asarray(recs.rec_off, dtype=np.uint64), np.asarray(recs.rec_len, dtype=np.uint64), fai, bases)


def fasta_counts(case):
    host = _fasta_host(case)
    return {"file_bytes": len(case["raw"]), "lines": case["raw"].count(b"\n") + 1, "headers": len(host.names), "bases": int(host.seq.size)}


def fasta_outcomes(case):
    host = _fasta_host(case)
    seq = np.asarray(host.seq)
    lower = (seq >= ord("a")) & (seq <= ord("z"))
    return {"a header": len(host.names) > 0, "a header with a description": b" record " in case["raw"], "a lower-case run": bool((lower[1:] & lower[:-1]).any()),
            "an N run": b"NN" in case["raw"], "a record of length 0": 0 in host.rec_len.tolist(), "a CRLF line": b"\r\n" in case["raw"]}


def expected_fasta(case):
    from tests.fasta_cases import codes
    host = _fasta_host(case)
    return _fasta_bytes(host, codes(np.asarray(host.seq).tobytes()))


def run_fasta(ctx, case):
    from ntsynt_amd import fasta as fa
    g, recs = fa.read_fasta_device(ctx, case["path"])
    try:
        return _fasta_bytes(recs, g.download(0, g.total_bp))
    finally:
        g.free()


def refuse_fasta(ctx, case):
    """the case's file with every '>' turned into '#': no header, as tests/test_gpu_fasta.py refuses it.  Found behind the scan: the file
    is uploaded ("fa_raw"), "fa_tile_nl", "fa_ctl" and "fa_hdr" are requested and k_fa_scan has run when the call returns NTS_EFORMAT.
    Through the C entry point, whose code Context.check turns into NtsError (fasta.read_fasta_device makes a ValueError of this one)"""
    import ctypes
    from ntsynt_amd import _lib
    path = _tmp_path("fasta_no_header.fa")
    with open(path, "wb") as fh:
        fh.write(case["raw"].replace(b">", b"#"))
    f, h = _lib.Fasta(), _lib.c_vp()
    rc = ctx.lib.nts_genome_from_fasta(ctx.h, os.fsencode(path), ctypes.byref(h), ctypes.byref(f))
    assert rc == -74 and not h.value, (rc, h.value)           # (NTS_EFORMAT; no genome was made)
    ctx.check(rc, "nts_genome_from_fasta")


def make_graph(size, seed):
    """three assemblies over one pool of hashes in one order with a few local reversals: most hashes in all three, some in two, some
    private, a few twice in one assembly (such a hash is no vertex); several records per assembly"""
    rng = np.random.default_rng(seed)
    n_pool, n_rec = (400, 3) if size == "S" else (2000, 12)
    pool = np.unique(rng.integers(1, U64_MAX, size=2 * n_pool, dtype=np.uint64))[:n_pool]
    rng.shuffle(pool)
    lists = []
    for a in range(3):
        order = np.arange(n_pool)
        for _ in range(n_pool // 50):                         # local reversals: edges that the assemblies do not share
            at = int(rng.integers(0, n_pool - 8))
            order[at:at + 6] = order[at:at + 6][::-1].copy()
        take = order[(rng.random(n_pool) < 0.85) | (order % 2 == 0)]           # (every even pool member is in all three)
        h = pool[take]
        dup = rng.choice(h.size, size=max(2, h.size // 60), replace=False)
        h[dup] = h[rng.choice(h.size, size=dup.size)]         # within-assembly repeats
        private = rng.integers(1, U64_MAX, size=h.size // 20, dtype=np.uint64)
        at = np.sort(rng.choice(h.size, size=private.size, replace=False))
        h = np.insert(h, at, private)
        rec = np.sort(rng.integers(0, n_rec, size=h.size)).astype(np.uint32)
        pos = np.zeros(h.size, dtype=np.uint64)
        for r in range(n_rec):
            m = rec == r
            pos[m] = np.cumsum(rng.integers(1, 400, size=int(m.sum()))).astype(np.uint64)
        lists.append((h, rec, pos))
    return {"lists": lists}


def _graph_ref(case):
    "tests/graph_ref.py's graph of the lists, its edges in the order the device hands them over (ntJoin's dict order)"
    if "ref" not in case:
        from ntsynt_amd.synteny import dict_order
        from tests.graph_ref import build_graph_numpy
        g = build_graph_numpy(case["lists"])
        order = dict_order(g.e_u, g.e_first, g.v_hash.size)
        case["ref"] = (g.v_hash, g.occ_rec, g.occ_pos, g.e_u[order], g.e_v[order], g.e_w[order], g.e_first[order])
    return case["ref"]


def _graph_bytes(cols):
    v_hash, rest = cols[0], cols[1:]
    return _cat(np.asarray(v_hash, dtype=np.uint64), *(np.asarray(x, dtype=np.int64) for x in rest))


def graph_counts(case):
    ref = _graph_ref(case)
    return {"minimizers": sum(x[0].size for x in case["lists"]), "vertices": int(ref[0].size), "edges": int(ref[3].size)}


def graph_outcomes(case):
    ref = _graph_ref(case)
    every = [set(x[0].tolist()) for x in case["lists"]]
    return {"a hash common to all assemblies": ref[0].size > 0, "a hash that is not": len(set.union(*every)) > len(set.intersection(*every)),
            "a hash twice in one assembly": any(len(s) < x[0].size for s, x in zip(every, case["lists"])), "an edge of weight above one": int(ref[5].max()) > 1,
            "an edge of weight one": int(ref[5].min()) == 1}


def expected_graph(case):
    return _graph_bytes(_graph_ref(case))


GRAPH_SLICES = 3                                              # the fewest hash slices the sliced entry's plan must have, at S and at L


def graph_budget(case):
    """bytes for the sliced build: a fifth of the elements per slice.  The library divides the budget by its own bytes per item
    (6 x 8 + 1 + the sort's temporary storage per item, under 70 in all: tests/test_gpu_graph_slices.py takes the same figure)"""
    return sum(x[0].size for x in case["lists"]) * 70 // 5


def run_graph(ctx, case):
    from ntsynt_amd.graph import build_graph_device
    ctx.set_graph_budget(0)
    g = build_graph_device(ctx, case["lists"])
    plan = ctx.graph_last_plan()
    assert plan["v_slices"] == 1 and plan["e_slices"] == 1, plan
    return _graph_bytes((g.v_hash, g.occ_rec, g.occ_pos, g.e_u, g.e_v, g.e_w, g.e_first))


def run_graph_sliced(ctx, case):
    "the budget is set before the call and 0 (automatic) after it: what a call leaves behind in the context is not the budget"
    from ntsynt_amd.graph import build_graph_device
    ctx.set_graph_budget(graph_budget(case))
    try:
        g = build_graph_device(ctx, case["lists"])
        plan = ctx.graph_last_plan()
    finally:
        ctx.set_graph_budget(0)
    case["sliced_plan"] = plan                                # (the last sliced build's plan of this case, for the test that prints it)
    assert plan["v_slices"] >= GRAPH_SLICES, plan
    return _graph_bytes((g.v_hash, g.occ_rec, g.occ_pos, g.e_u, g.e_v, g.e_w, g.e_first))


# ---- the other ways into a filter: one level of the cascade in place, the cascade into a second filter, the repeat filter ------------
def make_filters(size, seed):
    "a genome of 16 / 80 kbp with a stretch of it copied to another place (k-mers seen twice), and a relative 2 % away"
    k = 24
    rng, names, seqs = _genome(size, seed, 16_000, 80_000)
    first = bytearray(seqs[0])
    n = len(first) // 8
    first[5 * n:6 * n] = first[n:2 * n]
    seqs = [bytes(first)] + seqs[1:]
    og = to_oracle(names, seqs)
    relative = _mutated(rng, seqs, 0.02)
    return {"names": names, "seqs": seqs, "og": og, "relative": relative, "og2": to_oracle(names, relative), "k": k,
            "nbytes": O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.025))}


def _filters_brute(case):
    if "brute" not in case:
        first = O.bf_build(case["og"], case["k"], case["nbytes"])
        case["brute"] = {"first": first, "level": O.bf_build(case["og2"], case["k"], case["nbytes"], prev=first),
                         "repeat": O.repeat_bf([case["og"], case["og2"]], case["k"], case["nbytes"])}
    return case["brute"]


def filters_counts(case):
    return {"bases": case["og"].total_bp, "filter_bytes": case["nbytes"]}


def filters_outcomes(case):
    br = _filters_brute(case)
    return {"a bit that stays": O.bf_popcount(br["level"]) > 0, "a bit that goes": O.bf_popcount(br["level"]) < O.bf_popcount(br["first"]),
            "a k-mer seen twice": O.bf_popcount(br["repeat"]) > 0, "a k-mer seen once": O.bf_popcount(br["repeat"]) < O.bf_popcount(br["first"])}


def expected_bloom_and(case):
    level = _filters_brute(case)["level"]
    return _cat(level, np.array([O.bf_popcount(level)], dtype=np.uint64))


def expected_bloom_cascade(case):
    return _cat(_filters_brute(case)["level"], _filters_brute(case)["first"])


def expected_bloom_repeats(case):
    return _cat(_filters_brute(case)["repeat"])


def _with_filters(ctx, case, n_filters, call):
    "the genome and its relative resident, n_filters empty filters; the build on its binned way, as at the product's sizes"
    from ntsynt_amd.device import BloomFilter
    held = []
    ctx.bf_build_mode("binned")
    try:
        held += [to_device(ctx, case["names"], case["seqs"]), to_device(ctx, case["names"], case["relative"])]
        bfs = [BloomFilter(ctx, case["nbytes"], case["k"]) for _ in range(n_filters)]
        held += bfs
        return call(held[0], held[1], *bfs)
    finally:
        ctx.bf_build_mode("auto")
        for x in held:
            x.free()


def run_bloom_and(ctx, case):
    def call(g, rel, bf):
        bf.insert(g)
        bf.insert_and(rel)
        return _cat(bf.to_numpy(), np.array([bf.popcount()], dtype=np.uint64))
    return _with_filters(ctx, case, 1, call)


def run_bloom_cascade(ctx, case):
    def call(g, rel, prev, nxt):
        prev.from_numpy(_filters_brute(case)["first"])
        nxt.cascade_from(prev, rel)
        return _cat(nxt.to_numpy(), prev.to_numpy())
    return _with_filters(ctx, case, 2, call)


def run_bloom_repeats(ctx, case):
    "bin/ntsynt_make_repeat_bfs over the genome and its relative: one repeat filter, the genome's own filter cleared in between"
    def call(g, rel, rep, own):
        rep.insert_repeats_of(g, own)
        own.clear()
        rep.insert_repeats_of(rel, own)
        return _cat(rep.to_numpy())
    return _with_filters(ctx, case, 2, call)


# ---- the filter sweeps over intervals ------------------------------------------------------------------------------------------------
def make_filter_sweep(size, seed):
    "a genome of 6 / 30 kbp, the oracle's filter of a copy 5 % away, overlapping intervals over all records; one too short for a k-mer"
    k = 24
    rng, names, seqs = _genome(size, seed, 6_000, 30_000)
    n_iv = 6 if size == "S" else 36
    iv = []
    for i in range(n_iv):
        rec = i % len(seqs)
        start = int(rng.integers(0, len(seqs[rec]) - 400))
        iv.append((rec, start, start + int(rng.integers(200, 1200))))
    iv[1] = (iv[1][0], iv[1][1], iv[1][1] + k - 1)            # no k-mer: no hit
    og = to_oracle(names, seqs)
    nbytes = O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.025))
    return {"names": names, "seqs": seqs, "k": k, "iv": iv, "rate": 4, "bits": O.bf_build(to_oracle(names, _mutated(rng, seqs, 0.05)), k, nbytes)}


def _sweep_counts(case):
    if "counts" not in case:
        from tests.helpers import oracle_counts
        case["counts"] = oracle_counts(case["seqs"], case["k"], case["bits"], case["iv"])
    return case["counts"]


def _sweep_sample(case):
    "((records, per interval) against the filter, the same of every k-mer whatever holds it)"
    if "sample" not in case:
        from tests.helpers import oracle_sample
        ones = np.full(case["bits"].size, 0xFF, dtype=np.uint8)
        case["sample"] = (oracle_sample(case["seqs"], case["k"], case["bits"], case["iv"], case["rate"]),
                          oracle_sample(case["seqs"], case["k"], ones, case["iv"], case["rate"]))
    return case["sample"]


def sweep_counts(case):
    (recs, _), (every, _) = _sweep_sample(case)
    return {"intervals": len(case["iv"]), "bases": sum(len(s) for s in case["seqs"]), "filter_bytes": int(case["bits"].size), "records": int(recs.size),
            "records_unfiltered": int(every.size), "kmers": sum(n for n, _ in _sweep_counts(case))}


def sweep_outcomes(case):
    counts = _sweep_counts(case)
    per_iv = _sweep_sample(case)[0][1]
    return {"an interval with a hit": any(h > 0 for _, h in counts), "an interval without": any(h == 0 for _, h in counts),
            "a k-mer the filter does not hold": any(h < n for n, h in counts), "an interval with a record": bool((per_iv > 0).any()),
            "an interval without a record": bool((per_iv == 0).any())}


def expected_bf_count(case):
    counts = _sweep_counts(case)
    return _cat(np.array([n for n, _ in counts], dtype=np.uint64), np.array([h for _, h in counts], dtype=np.uint64))


def expected_bf_sample(case):
    (recs, per_iv), (every, every_iv) = _sweep_sample(case)
    return _cat(recs, per_iv, every, every_iv)


def _with_sweep(ctx, case, call):
    from ntsynt_amd.device import BloomFilter
    g = to_device(ctx, case["names"], case["seqs"])
    bf = None
    try:
        bf = BloomFilter(ctx, case["bits"].size, case["k"])
        bf.from_numpy(case["bits"])
        return call(g, bf)
    finally:
        if bf is not None:
            bf.free()
        g.free()


def run_bf_count(ctx, case):
    return _with_sweep(ctx, case, lambda g, bf: _cat(*g.bf_count_intervals(bf, case["iv"], case["k"])))


def run_bf_sample(ctx, case):
    "against the filter, then without one (nts_sample_intervals: the same host driver and scratch names)"
    return _with_sweep(ctx, case, lambda g, bf: _cat(*g.bf_sample_intervals(bf, case["iv"], case["k"], case["rate"]), *g.sample_intervals(case["iv"], case["k"], case["rate"])))


# ---- a minimizer list screened against a filter, and its k-mer text ------------------------------------------------------------------
def make_screen(size, seed):
    "the oracle's minimizers (w = 20) of a genome of 16 / 80 kbp; the filter: every other bit of the genome's own"
    k, w = 24, 20
    rng, names, seqs = _genome(size, seed, 16_000, 80_000)
    og = to_oracle(names, seqs)
    nbytes = O.bf_ctor_bytes(O.bf_approx_bytes(og.total_bp, 0.04))
    bits = np.unpackbits(O.bf_build(og, k, nbytes), bitorder="little")
    bits[rng.random(bits.size) < 0.5] = 0
    h1, rec, pos = oracle_flat(O.minimize(og, k, w))
    return {"names": names, "seqs": seqs, "k": k, "bits": np.packbits(bits, bitorder="little"), "mx": (h1.astype(np.uint64), rec.astype(np.uint32), pos.astype(np.uint64))}


def _screen_brute(case):
    "(which minimizers stay: the rule of tests/test_gpu_configs.py on the oracle's list; the k-mer text of all of them, upper case)"
    if "brute" not in case:
        k, (_, rec, pos) = case["k"], case["mx"]
        text = [case["seqs"][r][p:p + k].upper() for r, p in zip(rec.tolist(), pos.tolist())]
        keep = np.array([not O.bf_contains(case["bits"], O.hash_kmer(t)[0]) for t in text], dtype=bool)
        case["brute"] = (keep, np.frombuffer(b"".join(text), dtype=np.uint8))
    return case["brute"]


def expected_screen(case):
    keep, text = _screen_brute(case)
    return _cat(*(x[keep] for x in case["mx"]), text)


def run_screen(ctx, case):
    from ntsynt_amd.device import BloomFilter, Minimizers
    held = [to_device(ctx, case["names"], case["seqs"])]
    try:
        held.append(BloomFilter(ctx, case["bits"].size, case["k"]))
        held[1].from_numpy(case["bits"])
        held.append(Minimizers.from_numpy(ctx, *case["mx"]))
        held.append(held[2].screened(held[0], case["k"], held[1]))
        return _cat(*held[3].to_numpy(), held[2].kmers(held[0], case["k"]))
    finally:
        for x in held:
            x.free()


# ---- the pair counts of MinHash sketches ---------------------------------------------------------------------------------------------
def make_minhash_pairs(size, seed):
    "rows of up to s hashes from a small pool (pairs share some), an empty row, a copy of row 0, a row disjoint from all; every ordered pair of a seeded choice"
    rng = np.random.default_rng(seed)
    n_rows, s, n_pairs = (12, 32, 36) if size == "S" else (48, 128, 144)
    mult = np.uint64(0x9E3779B97F4A7C15 >> 12)
    rows = [np.unique(rng.choice(6 * s, size=int(rng.integers(1, s + 1)), replace=False)).astype(np.uint64) * mult for _ in range(n_rows)]
    rows[3] = np.zeros(0, dtype=np.uint64)
    rows[4] = rows[0].copy()
    rows[5] = rows[1] + np.uint64(1)
    pairs = [(0, 4), (5, 1), (3, 3), (3, 0), (0, 1)]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, n_rows, size=(n_pairs - len(pairs), 2))]
    return {"rows": rows, "s": s, "k": 21, "pairs": pairs}


def _pairs_brute(case):
    if "brute" not in case:
        from ntsynt_amd import divergence
        case["brute"] = [divergence.distance(case["rows"][a], case["rows"][b], case["k"], case["s"])[1:] for a, b in case["pairs"]]
    return case["brute"]


def pairs_outcomes(case):
    br = _pairs_brute(case)
    return {"an empty pair": any(sz == 0 for _, sz in br), "identical sketches": any(sh == sz > 0 for sh, sz in br), "disjoint sketches": any(sh == 0 < sz for sh, sz in br),
            "a partial overlap": any(0 < sh < sz for sh, sz in br)}


def expected_minhash_pairs(case):
    br = _pairs_brute(case)
    return _cat(np.array([sh for sh, _ in br], dtype=np.uint32), np.array([sz for _, sz in br], dtype=np.uint32))


def run_minhash_pairs(ctx, case):
    sk = np.zeros((len(case["rows"]), case["s"]), dtype=np.uint64)
    for i, r in enumerate(case["rows"]):
        sk[i, :r.size] = r
    return _cat(*ctx.minhash_pairs(sk, [r.size for r in case["rows"]], [a for a, _ in case["pairs"]], [b for _, b in case["pairs"]]))


# ======================================================================================================================================
# the catalogue
# ======================================================================================================================================
class Entry:
    """name; family: the shared scratch names it requests ("ivs_tmp" apart: ivs_tmp says whether it requests that one); group: entries of one group share one made case (the edit family's genome
    pair); make(size, seed); expected(case) -> bytes; run(ctx, case) -> bytes; counts(case) -> the dimensions that size its scratch;
    sizing: those of them L must hold four times over; outcomes(case) -> {what must occur: does it}; refuse(ctx, case): the entry's
    existing refused-arguments case, which raises NtsError (None: its tests have none)"""

    def __init__(self, name, family, group, make, expected, run, counts, sizing, outcomes, refuse=None):
        self.name, self.group, self.make, self.expected, self.run = name, group, make, expected, run
        self.ivs_tmp = "ivs_tmp" in family                    # requested by nearly every entry: met through the heavy partner, not pair by pair
        self.family = frozenset(family) - {"ivs_tmp"}
        self.counts, self.sizing, self.outcomes, self.refuse = counts, sizing, outcomes, refuse


def _edit_expected(what):
    def expected(case):
        br = _pair_brute(case)
        if what == "segments":
            return _identity_bytes(br["per_iv"], br["dist"])
        if what == "wide":
            return _identity_bytes(br["per_iv_wide"], br["final"])
        return _ops_bytes(br["ops"], br["first"]) if what == "script" else _ops_bytes(br["wops"], br["wfirst"])
    return expected


def _some(names, outcomes):
    return lambda case: {n: v for n, v in outcomes(case).items() if n in names}


IVS = ("ivs_tmp",)
ENTRIES = [
    Entry("edit_segments", EDIT_SHARED + ("edit_agg", "edit_out", "edit_uagg", "edit_uiv") + IVS, "pair", make_pair, _edit_expected("segments"),
          run_edit_segments, pair_counts, ("segments", "intervals", "bases"), _some(("aligned", "overband", "invalid", "passed"), pair_outcomes),
          refuse_edit_segments),
    Entry("edit_wide", EDIT_SHARED + ("edit_agg", "edit_out", "edit_uagg", "edit_uiv") + IVS, "pair", make_pair, _edit_expected("wide"), run_edit_wide,
          pair_counts, ("segments", "intervals", "work_set"), _some(("rescued offband", "rescued overband", "still passed", "invalid"), pair_outcomes),
          refuse_edit_wide),
    Entry("edit_script", EDIT_SHARED + SCRIPT_SHARED + IVS, "pair", make_pair, _edit_expected("script"), run_edit_script, pair_counts,
          ("segments", "intervals", "ops"), _some(("aligned", "passed", "script with an op"), pair_outcomes), refuse_edit_script),
    Entry("edit_wide_script", EDIT_SHARED + SCRIPT_SHARED + ("edit_taboff",) + IVS, "pair", make_pair, _edit_expected("wide_script"), run_edit_wide_script,
          pair_counts, ("segments", "intervals", "wide_ops"), _some(("wide member", "still passed", "aligned"), pair_outcomes), refuse_edit_wide_script),
    Entry("edit_extend", (), "world", make_world, expected_edit_extend, run_edit_extend, world_counts, ("tasks", "bases"), world_outcomes, refuse_edit_extend),
    Entry("edit_extend_script", ("edit_num",) + SCRIPT_SHARED + ("edit_taboff",) + IVS, "world", make_world, expected_edit_extend_script, run_edit_extend_script,
          world_counts, ("tasks", "ops"), world_outcomes, refuse_edit_extend_script),
    Entry("cigar_build", IVS, "cigar", make_cigar, expected_cigar_build, run_cigar_build, cigar_counts, ("pieces", "ops", "chains", "entries"), cigar_outcomes,
          refuse_cigar_build),
    Entry("cigar_lift", CIGX_SHARED + IVS, "lift", make_lift, expected_cigar_lift, run_cigar_lift, lift_counts, ("entries", "chains", "queries"), lift_outcomes,
          refuse_cigar_lift),
    Entry("cigar_lift_stats", CIGX_SHARED + IVS, "lift", make_lift, expected_cigar_lift_stats, run_cigar_lift_stats, lift_stats_counts,
          ("entries", "chains", "ranges"), lift_stats_outcomes, refuse_cigar_lift_stats),
    Entry("cigar_text", CIGX_SHARED + IVS, "lift", make_lift, expected_cigar_text, run_cigar_text, lift_text_counts, ("entries", "chains", "cg_bytes", "cs_bytes"),
          lift_text_outcomes, refuse_cigar_text),
    Entry("iv_anchor_segments", IVS, "anchors", make_anchor_segments, expected_anchor_segments, run_anchor_segments,
          lambda c: {"records_a": len(c["a"]), "records_b": len(c["b"]), "intervals": len(c["mate"]), "segments": len(_anchor_brute(c)[0])},
          ("records_a", "records_b", "intervals", "segments"),
          lambda c: {"a segment": len(_anchor_brute(c)[0]) > 0, "a record that is no anchor": sum(_anchor_brute(c)[1]) < len(c["a"])},
          lambda ctx, c: run_anchor_segments(ctx, c, band=0)),
    Entry("iv_links", (), "links", make_links, lambda c: _cat(_rows(LINK, _links_brute(c))), run_links,
          lambda c: {"records": sum(len(x) for x in c["lists"]), "links": len(_links_brute(c, 1)), "links_kept": len(_links_brute(c))}, ("records", "links", "links_kept"),
          lambda c: {"a link kept": len(_links_brute(c)) > 0, "a link dropped": len(_links_brute(c, 1)) > len(_links_brute(c)),
                     "a hash twice in one list": any(len({h for h, _, _ in x}) < len(x) for x in c["lists"])}),
    Entry("iv_sites", IVS, "sites", make_sites, lambda c: _cat(_rows(SITE, brute_sites(c["lists"], c["target"], c["step"], c["min_hits"]))), run_sites,
          lambda c: {"query_records": sum(x.size for x in c["lists"]), "target_records": int(c["target"].size),
                     "pairs": sum(s[3] for s in brute_sites(c["lists"], c["target"], c["step"], 1))}, ("query_records", "target_records", "pairs"),
          lambda c: {"a site kept": len(brute_sites(c["lists"], c["target"], c["step"], c["min_hits"])) > 0,
                     "a site dropped": len(brute_sites(c["lists"], c["target"], c["step"], 1)) > len(brute_sites(c["lists"], c["target"], c["step"], c["min_hits"]))},
          lambda ctx, c: run_sites(ctx, c, min_hits=0)),
    Entry("iv_periods", IVS, "periods", make_periods, expected_periods, lambda ctx, c: _cat(ctx.iv_periods(c["rec"], c["n_iv"])),
          lambda c: {"records": int(c["rec"].size), "intervals": c["n_iv"]}, ("records", "intervals"),
          lambda c: {"an interval with a period": any(r[2] > 0 for r in brute_periods(_triples(c["rec"]), c["n_iv"]))},
          lambda ctx, c: ctx.iv_periods(_beyond(c), c["n_iv"])),
    Entry("iv_period_hashes", IVF_SHARED + ("ivf_period",) + IVS, "period_hashes", make_period_hashes, expected_period_hashes,
          lambda ctx, c: _cat(ctx.iv_period_hashes(c["rec"], c["n_iv"], c["period"])),
          lambda c: {"records": int(c["rec"].size), "intervals": c["n_iv"]}, ("records", "intervals"),
          lambda c: {"a hash at its period": len(brute_period_hashes(_triples(c["rec"]), c["n_iv"], c["period"])) > 0},
          lambda ctx, c: ctx.iv_period_hashes(_beyond(c), c["n_iv"], c["period"])),
    Entry("iv_families", IVF_SHARED + IVS, "families", make_families, expected_families, run_families,
          lambda c: {"pairs": len(c["pairs"]), "arrays": c["n_arrays"], "hashes": len(brute_families(c["pairs"], c["n_arrays"])[1])}, ("pairs", "arrays", "hashes"),
          lambda c: {"two families": len(set(brute_families(c["pairs"], c["n_arrays"])[0])) >= 2,
                     "a family that joins arrays": max(np.bincount(brute_families(c["pairs"], c["n_arrays"])[0])) >= 2,
                     "an array of its own": 5 in brute_families(c["pairs"], c["n_arrays"])[0]},
          lambda ctx, c: run_families(ctx, c, n_arrays=max(a for _, a in c["pairs"]))),
    Entry("iv_family_sites", IVF_SHARED + IVS, "family_sites", make_family_sites, lambda c: _cat(as_sites(_family_sites_brute(c))), run_family_sites,
          lambda c: {"occurrences": int(c["occ"].size), "hashes": len(c["family_of"]), "sites": len(_family_sites_brute(c, 1))}, ("occurrences", "hashes", "sites"),
          lambda c: {"a site kept": len(_family_sites_brute(c)) > 0, "a site dropped": len(_family_sites_brute(c, 1)) > len(_family_sites_brute(c)),
                     "an occurrence that is no member": any(int(h) not in c["family_of"] for h in c["occ"]["h0"])},
          lambda ctx, c: run_family_sites(ctx, c, min_hits=0)),
    Entry("hset_sweep", ("hset_q", "hset_a", "hset_in"), "set", make_set_sweep, expected_set_sweep, run_set_sweep, set_counts, ("intervals", "members", "records", "bases"),
          lambda c: {"a k-mer in the set": _set_sample(c)[0].size > 0, "a query that is no member": not np.isin(c["queries"], c["members"]).all(),
                     "a k-mer outside it": _set_sample(c)[0].size < sum(int(((p >= s) & (p + c["k"] <= e)).sum()) for r, s, e in c["iv"] for p in [c["per_rec"][r][0]])},
          lambda ctx, c: run_set_sweep(ctx, c, iv=_bad_record(c))),
    Entry("hcount_capped", ("hset_q", "hset_a", "hset_in"), "set", make_set_sweep, expected_count_table, run_count_table, set_counts, ("intervals", "members", "records", "bases"),
          lambda c: {"a record kept": _count_brute(c)[2].size > 0, "a record over the cap": _count_brute(c)[2].size < _set_sample(c)[0].size,
                     "a count of zero read": 0 in _count_brute(c)[1], "a count above one read": int(_count_brute(c)[1].max()) > 1},
          lambda ctx, c: run_count_table(ctx, c, iv=_bad_record(c))),
    Entry("minhash", (), "minhash", make_minhash, expected_minhash, run_minhash, lambda c: {"bases": sum(len(s) for s in c["seqs"]), "hashes": c["s"]},
          ("bases", "hashes"), lambda c: {"a full sketch": len(expected_minhash(c)) == 8 * c["s"]}),
    Entry("minhash_intervals", (), "minhash", make_minhash, expected_minhash_intervals, run_minhash_intervals,
          lambda c: {"bases": sum(len(s) for s in c["seqs"]), "hashes": c["s"], "intervals": len(c["iv"])}, ("bases", "hashes", "intervals"),
          lambda c: {"a full sketch": any(h.size == c["s"] for h in oracle_sketches(c["seqs"], c["k"], c["s"], c["iv"])[0])},
          lambda ctx, c: run_minhash_intervals(ctx, c, iv=_bad_record(c))),
]
ENTRIES += [Entry("sketch_" + way, (), "sketch_" + way, make_sketch(way), expected_sketch, run_sketch, sketch_counts, ("bases", "minimizers", "filter_bytes"),
                  lambda c: {"minimizers": _sketch_brute(c)[0].size > 50,
                             "a rejected k-mer": int(np.unpackbits(c["bf"]).sum()) < sum(O.hash_all(s, c["k"])[1].size for s in c["seqs"])},
                  lambda ctx, c: run_sketch(ctx, c, w=WINDOW_LIMIT + 1))
            for way in SKETCH_WAYS]
ENTRIES += [
    Entry("bloom_insert", BIN_SHARED, "bloom", make_bloom, expected_bloom, run_bloom, lambda c: {"bases": c["og"].total_bp, "filter_bytes": c["nbytes"]},
          ("bases", "filter_bytes"), lambda c: {"bits set": np.unpackbits(O.bf_build(c["og"], c["k"], c["nbytes"])).sum() > 0}),
    Entry("engine_add_blocks", ("e_flag", "e_scan"), "engine", make_engine, expected_engine, run_engine, engine_counts, ("records", "minimizers", "vertices", "edges", "paths"),
          lambda c: {"a path": len(ES.oracle_trace(c)[0][-1][1]["paths"]) > 0, "a block": len(ES.oracle_trace(c)[0][-1][1]["rows"]) > 0}),
    # ---- the calls of every round (but for the FASTA parse, none of their tests refuses arguments)
    Entry("fasta_parse", (), "fasta", make_fasta, expected_fasta, run_fasta, fasta_counts, ("file_bytes", "lines", "headers", "bases"), fasta_outcomes,
          refuse_fasta),
    Entry("graph_build", GRAPH_SHARED, "graph", make_graph, expected_graph, run_graph, graph_counts, ("minimizers", "vertices", "edges"), graph_outcomes),
    Entry("graph_build_sliced", GRAPH_SHARED, "graph", make_graph, expected_graph, run_graph_sliced, graph_counts, ("minimizers", "vertices", "edges"), graph_outcomes),
    Entry("bloom_insert_and", BIN_SHARED, "filters", make_filters, expected_bloom_and, run_bloom_and, filters_counts, ("bases", "filter_bytes"),
          _some(("a bit that stays", "a bit that goes"), filters_outcomes)),
    Entry("bloom_cascade", BIN_SHARED, "filters", make_filters, expected_bloom_cascade, run_bloom_cascade, filters_counts, ("bases", "filter_bytes"),
          _some(("a bit that stays", "a bit that goes"), filters_outcomes)),
    Entry("bloom_repeats", (), "filters", make_filters, expected_bloom_repeats, run_bloom_repeats, filters_counts, ("bases", "filter_bytes"),
          _some(("a k-mer seen twice", "a k-mer seen once"), filters_outcomes)),
    Entry("bf_count_intervals", (), "filter_sweep", make_filter_sweep, expected_bf_count, run_bf_count, sweep_counts, ("intervals", "bases", "filter_bytes", "kmers"),
          _some(("an interval with a hit", "an interval without", "a k-mer the filter does not hold"), sweep_outcomes)),
    Entry("bf_sample_intervals", (), "filter_sweep", make_filter_sweep, expected_bf_sample, run_bf_sample, sweep_counts,
          ("intervals", "bases", "filter_bytes", "records", "records_unfiltered"), sweep_outcomes),
    Entry("mx_screen", (), "screen", make_screen, expected_screen, run_screen,
          lambda c: {"bases": sum(len(s) for s in c["seqs"]), "minimizers": int(c["mx"][0].size), "kept": int(_screen_brute(c)[0].sum()), "filter_bytes": int(c["bits"].size)},
          ("bases", "minimizers", "kept", "filter_bytes"),
          lambda c: {"a minimizer that stays": bool(_screen_brute(c)[0].any()), "a minimizer that goes": not _screen_brute(c)[0].all()}),
    Entry("minhash_pairs", (), "minhash_pairs", make_minhash_pairs, expected_minhash_pairs, run_minhash_pairs,
          lambda c: {"sketches": len(c["rows"]), "hashes": c["s"], "pairs": len(c["pairs"])}, ("sketches", "hashes", "pairs"), pairs_outcomes),
]
BY_NAME = {e.name: e for e in ENTRIES}
# where each entry's entry point requests its scratch (ntsynt_amd/csrc): what the host test reads the family table against
SOURCES = {"edit_segments": ["nts_edit.inc"], "edit_wide": ["nts_edit_wide.inc"], "edit_script": ["nts_edit_script.inc", "nts_edit_fr_script.inc"],
           "edit_wide_script": ["nts_edit_wide_script.inc", "nts_edit_fr_script.inc"], "edit_extend": ["nts_edit_extend.inc"],
           "edit_extend_script": ["nts_edit_extend_script.inc", "nts_edit_fr_script.inc"],
           "cigar_build": ["nts_cigar.inc"], "cigar_lift": ["nts_cigar.inc"], "cigar_lift_stats": ["nts_cigar.inc"],
           "cigar_text": ["nts_cigar.inc"], "iv_anchor_segments": ["nts_iv_anchors.inc"], "iv_links": ["nts_iv_links.inc"],
           "iv_sites": ["nts_iv_sites.inc"], "iv_periods": ["nts_iv_periods.inc"], "iv_period_hashes": ["nts_iv_families.inc"],
           "iv_families": ["nts_iv_families.inc"], "iv_family_sites": ["nts_iv_families.inc"], "hset_sweep": ["nts_hset.inc"],
           "hcount_capped": ["nts_hset.inc", "nts_hcount.inc"], "minhash": ["nts_minhash.inc"], "minhash_intervals": ["nts_minhash_iv.inc"],
           "bloom_insert": ["ntsynt_hip.hip", "nts_bloom_bin.inc"], "engine_add_blocks": ["nts_dgraph.inc"]}
SOURCES.update({"sketch_" + way: ["ntsynt_hip.hip", "nts_pruned.inc", "nts_tiers.inc"] for way in SKETCH_WAYS})
SOURCES.update({"fasta_parse": ["nts_fasta_dev.inc"], "graph_build": ["nts_graph.hip"], "graph_build_sliced": ["nts_graph.hip"],
                "bloom_insert_and": ["ntsynt_hip.hip", "nts_bloom_bin.inc"], "bloom_cascade": ["ntsynt_hip.hip", "nts_bloom_bin.inc"],
                "bloom_repeats": ["ntsynt_hip.hip", "nts_bloom_bin.inc"], "bf_count_intervals": ["nts_bf_iv.inc"], "bf_sample_intervals": ["nts_bf_sample.inc"],
                "mx_screen": ["nts_dgraph.inc", "nts_fasta_dev.inc"], "minhash_pairs": ["nts_minhash_iv.inc"]})
# the library's exported functions that an entry's run() calls and that request scratch in nts_graph.hip, nts_fasta_dev.inc, nts_bf_iv.inc or
# nts_bf_sample.inc, themselves or through a helper (tests/test_call_order_cases_host.py reads the sources for them; the exchanges of
# nts_comm.inc are the rank test's: tests/test_gpu_call_order_ranks.py)
CALLS = {"fasta_parse": ["nts_genome_from_fasta"], "graph_build": ["nts_graph_build"], "graph_build_sliced": ["nts_graph_build"],
         "engine_add_blocks": ["nts_engine_add"], "bf_count_intervals": ["nts_bf_count_intervals"],
         "bf_sample_intervals": ["nts_bf_sample_intervals", "nts_sample_intervals"], "mx_screen": ["nts_mx_screen", "nts_mx_kmers"],
         "hset_sweep": ["nts_hset_sample_intervals"], "hcount_capped": ["nts_hset_sample_intervals_capped"]}
STAGED = ["sketch_" + way for way in SKETCH_WAYS]               # the calls that go through upload_packed's pinned staging area (ntsynt_hip.hip)
HEAVY_PARTNER = "iv_family_sites"                             # every entry also runs around this one at L: the busiest user of "ivs_tmp"
# ordered pairs beyond the family table: the sliced build drops scratch that the one-pass build and the engine keep ("e_hook_a", "e_hook_b",
# "e_scan_tmp" are the engine's names; the engine's add runs the build's passes on the g_* / gs_* names), the FASTA parse shares the pinned
# staging area with every way of the sketch, the repeat filter goes the Bloom build's other way, the two filter sweeps share their tile cutter
PAIRED = [("graph_build_sliced", "engine_add_blocks"), ("engine_add_blocks", "graph_build_sliced"), ("engine_add_blocks", "graph_build"),
          ("bloom_insert", "bloom_repeats"), ("bloom_repeats", "bloom_insert"), ("bf_count_intervals", "bf_sample_intervals"),
          ("bf_sample_intervals", "bf_count_intervals")]
PAIRED += [pair for way in SKETCH_WAYS for pair in (("fasta_parse", "sketch_" + way), ("sketch_" + way, "fasta_parse"))]

_cases, _expected = {}, {}


def case_of(name, size):
    "the entry's case at a size: made once per group and size, left unchanged"
    e = BY_NAME[name]
    key = (e.group, size)
    if key not in _cases:
        _cases[key] = e.make(size, SEED[size] + sum(map(ord, e.group)))
    return _cases[key]


def expected_of(name, size):
    if (name, size) not in _expected:
        _expected[(name, size)] = BY_NAME[name].expected(case_of(name, size))
    return _expected[(name, size)]


def neighbours():
    "ordered pairs (X, Y) whose families meet or that share the staging area, the pairs listed by hand (PAIRED), and every entry with the heavy partner"
    out = [(x.name, y.name) for x in ENTRIES for y in ENTRIES if x is not y and x.family & y.family]
    out += [(x, y) for x in STAGED for y in STAGED if x != y]
    out += [p for p in PAIRED if p not in out]
    return out + [(e.name, HEAVY_PARTNER) for e in ENTRIES if (e.name, HEAVY_PARTNER) not in out and e.name != HEAVY_PARTNER]


# ---- the long chain ------------------------------------------------------------------------------------------------------------------
CHAIN_SEED, CHAIN_PASSES = 123391, 3                         # (the smallest seed that leaves out no entry and no size: tests/test_call_order_cases_host.py checks it)


def chain_order(seed=CHAIN_SEED, passes=CHAIN_PASSES):
    "[(name, size)]: every entry once per pass in a seeded shuffled order, each at a seeded choice of S or L"
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(passes):
        names = [e.name for e in ENTRIES]
        rng.shuffle(names)
        out += [(n, SIZES[int(rng.integers(0, 2))]) for n in names]
    return out

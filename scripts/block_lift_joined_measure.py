#!/usr/bin/env python3
"""Device time of the joined lift (docs/design/04_27_lift_joined.md) beside the per-chain counts of the lift identity, on the measurement
input of docs/design/04_22_block_alignments.md run with E = 0 and without ends -- so that the chains of a pair break at the indels wider
than the band; with E = 1023 every pair there has one chain and nothing is joined -- and on the interval grid of
docs/design/04_23_block_lift.md (`--width`-base intervals every `--step` bases of the aligned target) plus windows of `--window` bases
over genome 0.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit:
lift_pairs_scan and lift_pairs_search of nts_cigar_lift_pairs beside lift_stats_scan and lift_stats_search of nts_cigar_lift_stats on the
same intervals; the chains per pair; the host time of lift_pair_ranges beside lift_queries + lift_ranges, once.  Output:
profiles/block_lift_joined_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd import assess  # noqa: E402
from ntsynt_amd.device import LIFT_LINK_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402

STATS_TIMERS = ["lift_stats_scan", "lift_stats_search"]
PAIRS_TIMERS = ["lift_pairs_scan", "lift_pairs_search"]


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--width", type=int, default=100)
    p.add_argument("--step", type=int, default=16)
    p.add_argument("--window", type=int, default=1000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_lift_joined_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    seq_a, seq_b, iv_a, iv_b = family(bp, args.intervals, args.every, np.random.default_rng(SEED))
    ctx = Context(0)
    ctx.profile(True)
    zero = np.zeros(1, dtype=np.uint64)
    g_a = Genome(ctx, ["a"], seq_a, zero, np.array([seq_a.size], dtype=np.uint64))
    g_b = Genome(ctx, ["b"], seq_b, zero, np.array([seq_b.size], dtype=np.uint64))
    n_iv = iv_a.shape[0]
    rec_a, _ = g_a.sample_intervals(iv_a, K, RATE)
    rec_b, _ = g_b.sample_intervals(iv_b, K, RATE)
    mate = np.arange(n_iv, dtype=np.uint32)
    len_b = (iv_b[:, 2] - iv_b[:, 1]).astype(np.uint32)
    flip = np.zeros(n_iv, dtype=np.uint8)
    lines = [(i, i, i) for i in range(n_iv)]
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)     # E = 0: the narrow band alone, no flanks
    narrow = ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist)
    pieces, source, chains = assess.alignment_pieces(segs, dist, lines)
    ops, first = assess.alignment_ops(source, [narrow])
    n_chains = int(chains["line"].size)
    cigar, records = ctx.cigar_build(pieces, ops, first, n_chains)
    line = chains["line"]
    order = np.argsort(line, kind="stable")
    start_a, start_b = iv_a[line[order], 1].astype(np.int64), iv_b[line[order], 1].astype(np.int64)
    spans = {"pair": line[order], "chain": order, "side": np.zeros(order.size, dtype=np.int64), "flip": np.zeros(order.size, dtype=bool),
             "contig": ["a"] * order.size, "s0": start_a + chains["x0"][order], "s1": start_a + chains["x1"][order],
             "o0": start_b + chains["y0"][order], "o1": start_b + chains["y1"][order]}
    # the links: the chains with entries in (pair, ch) order at their oriented offsets (every pair is `+`, every interval on record 0)
    linked = np.flatnonzero(records["n_cig"][order] > 0)
    links = np.zeros(linked.size, dtype=LIFT_LINK_DTYPE)
    links["chain"], links["a0"], links["b0"] = order[linked], chains["x0"][order][linked], chains["y0"][order][linked]
    of_line = line[order][linked]
    pair_first = np.searchsorted(of_line, np.arange(n_iv + 1)).astype(np.uint64)
    per_pair = np.diff(pair_first.astype(np.int64))
    has = per_pair > 0
    first_link, last_link = np.minimum(pair_first[:-1].astype(np.int64), linked.size - 1), np.maximum(pair_first[1:].astype(np.int64) - 1, 0)
    pairs = {"side": np.zeros(n_iv, dtype=np.int64), "flip": np.zeros(n_iv, dtype=bool), "contig": ["a"] * n_iv, "origin": iv_a[:, 1].astype(np.int64),
             "h0": np.where(has, chains["x0"][order][linked][first_link], 0), "h1": np.where(has, chains["x1"][order][linked][last_link], 0)}
    lo, hi = int(spans["s0"].min()), int(spans["s1"].max())
    grid = np.arange(lo, hi - args.width, args.step, dtype=np.int64)
    sets = {"grid": {"contig": ["a"] * grid.size, "name": ["."] * grid.size, "start": grid, "end": grid + args.width},
            "windows": assess.window_intervals([("a", int(seq_a.size))], args.window)}
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": 0, "ends": None,
           "chains": n_chains, "links": int(links.size), "pairs": int(n_iv), "entries": int(cigar.size),
           "chains_per_pair": {"min": int(per_pair.min()), "median": float(np.median(per_pair)), "mean": float(per_pair.mean()), "max": int(per_pair.max())},
           "aligned_bases_a": int(records["len_a"].sum()), "grid_width": args.width, "grid_step": args.step, "window": args.window, "calls": args.calls}
    for name, intervals in sets.items():
        host = {}
        t0 = time.perf_counter()
        queries, overlaps = assess.lift_queries(spans, intervals)
        host["lift_queries_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ranges, _ = assess.lift_ranges(queries, overlaps)
        host["lift_ranges_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        pair_ranges, which = assess.lift_pair_ranges(pairs, intervals)
        host["lift_pair_ranges_ms"] = (time.perf_counter() - t0) * 1e3
        stats = ctx.cigar_lift_stats(cigar, records, ranges)                                        # warm-up, and the results
        joined = ctx.cigar_lift_pairs(cigar, records, links, pair_first, pair_ranges)
        both = joined["eq"] + joined["x"]
        assert np.array_equal(both + joined["src_gap"] + joined["src_open"], joined["src_hi"] - joined["src_lo"])
        assert np.array_equal(both + joined["oth_gap"] + joined["oth_open"], joined["oth_hi"] - joined["oth_lo"])
        adds_up = bool(int(joined["eq"].sum()) == int(stats["eq"].sum()) and int(joined["n_links"].sum()) == int(ranges.size))    # (the per-chain lines, added up)

        def calls():
            ctx.cigar_lift_stats(cigar, records, ranges)
            ctx.cigar_lift_pairs(cigar, records, links, pair_first, pair_ranges)
        t = timed(ctx, STATS_TIMERS + PAIRS_TIMERS, calls, args.calls)
        per_call_ms = {}
        for timer in STATS_TIMERS + PAIRS_TIMERS:
            scopes = t[timer]["timed_launches_per_call"]
            assert len(scopes) == 1, (timer, scopes)
            per_call_ms[timer] = t[timer]["median_ms"] * scopes[0]
        stats_ms, pairs_ms = (sum(per_call_ms[timer] for timer in timers) for timers in (STATS_TIMERS, PAIRS_TIMERS))
        out[name] = dict(t, n_intervals=len(intervals["contig"]), per_chain_ranges=int(ranges.size), pair_ranges=int(pair_ranges.size),
                         joined_lines=int(np.count_nonzero(joined["n_links"])), joined_lines_of_several_chains=int(np.count_nonzero(joined["n_links"] > 1)),
                         per_call_ms=per_call_ms, stats_per_call_ms=stats_ms, pairs_per_call_ms=pairs_ms, pairs_over_stats=pairs_ms / stats_ms if stats_ms else None,
                         matches_and_chains_add_up_to_the_per_chain_lines=adds_up, host_ms=host)
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

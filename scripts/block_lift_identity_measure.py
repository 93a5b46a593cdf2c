#!/usr/bin/env python3
"""Device time of the alignment counts of the lift identity (docs/design/04_25_lift_identity.md) beside the coordinate map of the block
lift, on the measurement input of docs/design/04_22_block_alignments.md and the interval grid of docs/design/04_23_block_lift.md
(scripts/block_lift_measure.py: `--width`-base intervals every `--step` bases of the aligned target), plus windows of `--window` bases
over genome 0 on the same input.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a
time limit: lift_stats_scan and lift_stats_search of nts_cigar_lift_stats beside lift_scan and lift_search of nts_cigar_lift in the same
calls -- the parent's way to the two end points of the same intervals --, for the grid and for the windows; entries, chains,
intervals, overlaps; the host time of lift_queries, lift_ranges and lift_rows, once (the Python loop that makes the table's lines is not
timed).  Output: profiles/block_lift_identity_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd import assess  # noqa: E402
from ntsynt_amd.device import Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_EDITS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402

LIFT_TIMERS = ["lift_scan", "lift_search"]
STATS_TIMERS = ["lift_stats_scan", "lift_stats_search"]


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
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_lift_identity_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    cap, limit, penalty = assess.ENDS_MAX_LEN, assess.ENDS_MAX_EDITS, assess.ENDS_PENALTY
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
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)
    _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
    tasks, flanks = assess.ends_tasks(segs, final, iv_a, iv_b, flip, lines, g_a.rec_len, g_b.rec_len, cap)
    results = ctx.edit_extend(g_a, g_b, tasks, penalty, limit)
    narrow = ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist)
    wide = ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final)
    flank_script = ctx.edit_extend_script(g_a, g_b, tasks, results)
    pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
    ops, first = assess.alignment_ops(source, [narrow, wide], flank_script)
    n_chains = int(chains["line"].size)
    cigar, records = ctx.cigar_build(pieces, ops, first, n_chains)
    # the chains' forward spans, as block_lift makes them (every pair is `+`, every interval on record 0)
    line = chains["line"]
    order = np.argsort(line, kind="stable")
    start_a, start_b = iv_a[line[order], 1].astype(np.int64), iv_b[line[order], 1].astype(np.int64)
    spans = {"pair": line[order], "chain": order, "side": np.zeros(order.size, dtype=np.int64), "flip": np.zeros(order.size, dtype=bool),
             "contig": ["a"] * order.size, "s0": start_a + chains["x0"][order], "s1": start_a + chains["x1"][order],
             "o0": start_b + chains["y0"][order], "o1": start_b + chains["y1"][order]}
    lo, hi = int(spans["s0"].min()), int(spans["s1"].max())
    grid = np.arange(lo, hi - args.width, args.step, dtype=np.int64)
    sets = {"grid": {"contig": ["a"] * grid.size, "name": ["."] * grid.size, "start": grid, "end": grid + args.width},
            "windows": assess.window_intervals([("a", int(seq_a.size))], args.window)}
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "ends_max_len": cap, "ends_max_edits": limit, "ends_penalty": penalty, "chains": n_chains, "entries": int(cigar.size),
           "entries_per_chain_max": int(records["n_cig"].max()), "aligned_bases_a": int(records["len_a"].sum()), "grid_width": args.width,
           "grid_step": args.step, "window": args.window, "calls": args.calls}
    for name, intervals in sets.items():
        host = {}
        t0 = time.perf_counter()
        queries, overlaps = assess.lift_queries(spans, intervals)
        host["lift_queries_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ranges, which = assess.lift_ranges(queries, overlaps)
        host["lift_ranges_ms"] = (time.perf_counter() - t0) * 1e3
        hits = ctx.cigar_lift(cigar, records, queries)                                              # warm-up, and the results
        stats = ctx.cigar_lift_stats(cigar, records, ranges)
        t0 = time.perf_counter()
        rows = assess.lift_rows(spans, overlaps, hits)
        host["lift_rows_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(stats["oth_hi"] - stats["oth_lo"], (rows["to_end"] - rows["to_start"]).astype(np.uint64))
        assert np.array_equal(stats["eq"] + stats["x"] + stats["src_gap"], ranges["hi"] - ranges["lo"])

        def both():
            ctx.cigar_lift(cigar, records, queries)
            ctx.cigar_lift_stats(cigar, records, ranges)
        t = timed(ctx, LIFT_TIMERS + STATS_TIMERS, both, args.calls)
        per_call_ms = {}
        for timer in LIFT_TIMERS + STATS_TIMERS:
            scopes = t[timer]["timed_launches_per_call"]
            assert len(scopes) == 1, (timer, scopes)
            per_call_ms[timer] = t[timer]["median_ms"] * scopes[0]
        lift_ms, stats_ms = (sum(per_call_ms[timer] for timer in timers) for timers in (LIFT_TIMERS, STATS_TIMERS))
        out[name] = dict(t, n_intervals=len(intervals["contig"]), overlaps=int(overlaps["interval"].size), queries=int(queries.size), ranges=int(ranges.size),
                         identity_mean=float(stats["eq"].sum()) / float((stats["eq"] + stats["x"] + stats["src_gap"] + stats["oth_gap"]).sum()),
                         per_call_ms=per_call_ms, lift_per_call_ms=lift_ms, stats_per_call_ms=stats_ms, stats_over_lift=stats_ms / lift_ms if lift_ms else None,
                         stats_scan_over_lift_scan=per_call_ms["lift_stats_scan"] / per_call_ms["lift_scan"] if per_call_ms["lift_scan"] else None,
                         stats_search_over_lift_search=per_call_ms["lift_stats_search"] / per_call_ms["lift_search"] if per_call_ms["lift_search"] else None,
                         host_ms=host)
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

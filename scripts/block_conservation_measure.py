#!/usr/bin/env python3
"""Device time of nts_cigar_depth, the call behind `--block-conservation` (docs/design/04_31_block_conservation.md), on the input and by
the method of scripts/block_maf_multi_measure.py: a reference of `--bp` bases and two queries derived from it with indels `--every` and
`--every` + 700 bases apart, `--intervals` blocks, at E = 0 without ends; the core chains of the two star pairs.  One process, device
events (the library's timers, summed per call: cigar_depth_events and cigar_depth_emit are opened twice each in one call), medians of
six calls with minimum and maximum, a time limit; the host clock of the call and of the NumPy difference-array rendering of the same
segments (assess.depth_segments_host per group), the bytes compared.  Output: profiles/block_conservation_measure.json.  Needs the GPU:
there is no fallback."""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd import assess  # noqa: E402
from ntsynt_amd.device import CHAIN_DTYPE, CIG_DEPTH_SEG_DTYPE, CIG_PAD_AT_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.block_maf_multi_measure import cores_of  # noqa: E402

TIMERS = ["cigar_depth_events", "cigar_depth_emit"]


def host_segments(entries, records, at, n_groups):
    "the segments of every group by assess.depth_segments_host, as nts_cigar_depth returns them"
    cut = np.searchsorted(at["group"], np.arange(n_groups + 1))
    parts, seg_first = [], np.zeros(n_groups + 1, dtype=np.uint64)
    for g in range(n_groups):
        lo, hi = int(cut[g]), int(cut[g + 1])
        if hi > lo:
            e_lo, e_hi = int(records["first"][lo]), int(records["first"][hi - 1] + records["n_cig"][hi - 1])
            sub = records[lo:hi].copy()
            sub["first"] -= e_lo
            start, end, aligned, match, gap = assess.depth_segments_host(entries[e_lo:e_hi], sub, at[lo:hi])
            part = np.zeros(start.size, dtype=CIG_DEPTH_SEG_DTYPE)
            part["start"], part["end"], part["group"], part["aligned"], part["match"], part["gap"] = start, end, g, aligned, match, gap
            parts.append(part)
        seg_first[g + 1] = seg_first[g] + (parts[-1].size if hi > lo else 0)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=CIG_DEPTH_SEG_DTYPE)), seg_first


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=540)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_conservation_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    seq_a, seq_b, iv_a, iv_b = family(bp, args.intervals, args.every, np.random.default_rng(SEED))
    again, seq_c, _, iv_c = family(bp, args.intervals, args.every + 700, np.random.default_rng(SEED))
    assert np.array_equal(seq_a, again), "the third genome must derive from the same reference"
    ctx = Context(0)
    ctx.profile(True)
    zero = np.zeros(1, dtype=np.uint64)
    genomes = [Genome(ctx, [n], s, zero, np.array([s.size], dtype=np.uint64)) for n, s in (("a", seq_a), ("b", seq_b), ("c", seq_c))]
    held = []                                                 # (group, row, t0, entries, len_a, len_b, pos_b)
    for row, (g, iv) in enumerate(((genomes[1], iv_b), (genomes[2], iv_c)), 1):
        held += [(c[0], row) + c[1:] for c in cores_of(ctx, genomes[0], g, iv_a, iv)]
    held.sort(key=lambda h: h[:3])
    entries = np.concatenate([h[3] for h in held]).astype(np.uint64)
    records = np.zeros(len(held), dtype=CHAIN_DTYPE)
    records["n_cig"] = [h[3].size for h in held]
    records["first"] = np.concatenate(([0], np.cumsum(records["n_cig"][:-1].astype(np.int64))))
    records["len_a"], records["len_b"] = [h[4] for h in held], [h[5] for h in held]
    at = np.zeros(len(held), dtype=CIG_PAD_AT_DTYPE)
    at["group"], at["t0"] = [h[0] for h in held], [h[2] for h in held]
    n_groups = int(iv_a.shape[0])
    segs, seg_first = ctx.cigar_depth(entries, records, at, n_groups)          # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, want_first = host_segments(entries, records, at, n_groups)
        host.append((time.perf_counter() - t0) * 1e3)
    assert segs.tobytes() == want.tobytes() and seg_first.tobytes() == want_first.tobytes(), "the device's segments are not the host's"
    per_call, clock = {t: [] for t in TIMERS}, []
    for _ in range(args.calls):
        before = {t: ctx.timing(t)[0] for t in TIMERS}
        t0 = time.perf_counter()
        again_segs, again_first = ctx.cigar_depth(entries, records, at, n_groups)
        clock.append((time.perf_counter() - t0) * 1e3)
        assert again_segs.tobytes() == segs.tobytes() and again_first.tobytes() == seg_first.tobytes()
        for t in TIMERS:
            per_call[t].append(ctx.timing(t)[0] - before[t])

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}
    rows = np.full(n_groups, 2)
    summary = assess.conservation_summary(segs, seg_first, rows)
    consuming = int(np.isin(entries & np.uint64(15), [2, 7, 8]).sum())
    out = {"bp": bp, "intervals": n_groups, "indel_every": [args.every, args.every + 700], "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN,
           "chains": len(held), "entries": int(entries.size), "consuming_entries": consuming, "events": consuming + len(held),
           "insertion_entries": int(((entries & np.uint64(15)) == np.uint64(1)).sum()),
           "segments": int(segs.size), "most_aligned": int(segs["aligned"].max()) if segs.size else 0,
           "covered": sum(s["covered"] for s in summary), "core": sum(s["core"] for s in summary), "conserved": sum(s["conserved"] for s in summary),
           "calls": args.calls, "per_call_ms": {t: spread(per_call[t]) for t in TIMERS}, "host_call_ms": spread(clock),
           "host_numpy_segments_ms": spread(host)}
    for g in genomes:
        g.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device times of the wide pass of the block identity beside the narrow one (docs/design/04_18_block_identity_wide.md) on two genomes
of one ancestor made on the host: `--bp` bases in `--intervals` tiles, tile i of one genome the mate of tile i of the other, 1 %
substitutions and one indel of 32 - 300 bases every `--every` bases (half insertions, half deletions), k 21, rate 16, band 31,
max_len 4096, E 1023.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit.
The timers edit_segments, edit_wide_plan and edit_wide on the same segments; the size of the work set and what became of it; work-set
segments per second and the cells of their full tables per second; the ratio edit_wide / edit_segments.
Output: profiles/block_identity_wide_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import EDIT_INVALID, EDIT_OVERBAND, EDIT_PASSED, SEG_OFFBAND, Context, Genome  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402

SEED, DIVERGENCE = 20240207, 0.01
K, RATE, BAND, MAX_LEN, MAX_EDITS = 21, 16, 31, 4096, 1023
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def family(bp, tiles, every, rng):
    "(sequence of A, sequence of B, intervals of A, intervals of B): B = A with substitutions and, per tile, indels `every` bases apart"
    a = LETTERS[rng.integers(0, 4, size=bp)]
    b = a.copy()
    hit = np.flatnonzero(rng.random(bp) < DIVERGENCE)
    b[hit] = LETTERS[(np.searchsorted(LETTERS, b[hit]) + rng.integers(1, 4, size=hit.size)) % 4]
    step = -(-bp // tiles)
    pieces, iv_a, iv_b, at_b = [], [], [], 0
    for s in range(0, bp, step):
        e, size = min(s + step, bp), 0
        at = s
        for where in range(s + every // 2, e - 400, every):
            n = int(rng.integers(32, 301))
            pieces.append(b[at:where])
            size += where - at
            if rng.random() < 0.5:
                pieces.append(LETTERS[rng.integers(0, 4, size=n)])
                size += n
                at = where
            else:
                at = where + n
        pieces.append(b[at:e])
        size += e - at
        iv_a.append((0, s, e))
        iv_b.append((0, at_b, at_b + size))
        at_b += size
    return a, np.concatenate(pieces), np.array(iv_a, dtype=np.uint64), np.array(iv_b, dtype=np.uint64)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_identity_wide_measure.json"))
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
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)
    narrow_iv, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)          # warm-up, and the distances
    wide_iv, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
    gap = np.abs(segs["dy"].astype(np.int64) - segs["dx"].astype(np.int64))
    work = ((segs["kind"] == SEG_OFFBAND) & (dist == EDIT_PASSED) & (gap <= MAX_EDITS)) | (dist == EDIT_OVERBAND)
    cells = int((segs["dx"][work].astype(np.int64) * segs["dy"][work].astype(np.int64)).sum())
    t_seg = timed(ctx, ["edit_segments", "edit_reduce"], lambda: ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True), args.calls)
    t_wide = timed(ctx, ["edit_wide_plan", "edit_wide", "edit_reduce"], lambda: ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist),
                   args.calls)
    seconds = t_wide["edit_wide"]["median_ms"] * 1e-3
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "segments": int(segs.size), "narrow_aligned_segments": int((dist < EDIT_INVALID).sum()), "narrow_edits": int(narrow_iv["edits"].sum()),
           "work_set": int(work.sum()), "work_set_offband": int((work & (segs["kind"] == SEG_OFFBAND)).sum()),
           "work_set_aligned": int((work & (final < EDIT_INVALID)).sum()), "work_set_still_overband": int((work & (final == EDIT_OVERBAND)).sum()),
           "work_set_edits": int(final[work & (final < EDIT_INVALID)].sum()), "wide_edits": int(wide_iv["edits"].sum()),
           "work_set_bases_a": int(segs["dx"][work].sum()), "work_set_table_cells": cells,
           "edit_segments": t_seg, "edit_wide": t_wide,
           "work_set_segments_per_second": int(work.sum()) / seconds, "table_cells_equivalent_per_second": cells / seconds,
           "edit_wide_over_edit_segments": t_wide["edit_wide"]["median_ms"] / t_seg["edit_segments"]["median_ms"]}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

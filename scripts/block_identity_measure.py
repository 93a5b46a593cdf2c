#!/usr/bin/env python3
"""Device times of the block identity's two calls (docs/design/04_16_block_identity.md) on two synthetic genomes of one ancestor:
`--bp` bases each (3 Gbp by default) at 1 % divergence, tiled by 10^4 intervals, interval i of one genome the mate of interval i of the
other, k 21, rate 16, band 31, max_len 4096.  One process, device events (the library's timers), medians of six calls with minimum
and maximum, a time limit.  Per call: anchors, segments, aligned bases, the cells nts_edit_segments' kernel updates per second
(every aligned or overband segment steps dx + dy antidiagonals of 2 W + 1 diagonals, half of them live per step), every timer, and
nts_iv_links on the same two lists beside the anchor join.  Output: profiles/block_identity_measure.json.  Needs the GPU: there is no
fallback."""
import argparse
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import EDIT_INVALID, EDIT_OVERBAND, SEG_CANDIDATE, Context, Genome  # noqa: E402
from scripts.gap_links_measure import tiling, timed  # noqa: E402

SEED, DIVERGENCE = 20240207, 0.01
K, RATE, BAND, MAX_LEN = 21, 16, 31, 4096


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=3e9)
    p.add_argument("--contigs", type=int, default=24)
    p.add_argument("--intervals", type=int, default=10_000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=1100)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_identity_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    ctx = Context(0)
    ctx.profile(True)
    bp = int(args.bp)
    g_a = Genome.synth(ctx, bp, args.contigs, SEED, 1, DIVERGENCE)
    g_b = Genome.synth(ctx, bp, args.contigs, SEED, 2, DIVERGENCE)
    iv = tiling(g_a, args.intervals)
    n_iv = iv.shape[0]
    rec_a, _ = g_a.sample_intervals(iv, K, RATE)
    rec_b, _ = g_b.sample_intervals(iv, K, RATE)
    mate = np.arange(n_iv, dtype=np.uint32)
    len_b = (iv[:, 2] - iv[:, 1]).astype(np.uint32)
    flip = np.zeros(n_iv, dtype=np.uint8)
    out = {"bp": bp, "intervals": int(n_iv), "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "records": [int(rec_a.size), int(rec_b.size)]}
    segs, anchors = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)      # warm-up, and the counts
    out["iv_anchor_segments"] = dict(timed(ctx, ["iv_anchors_join", "iv_anchors_segments"],
                                           lambda: ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN), args.calls),
                                     anchors=int(anchors.sum()), segments=int(segs.size), candidates=int((segs["kind"] == SEG_CANDIDATE).sum()))
    links = ctx.iv_links([rec_a, rec_b], 1)
    out["iv_links_same_lists"] = dict(timed(ctx, ["iv_links_join", "iv_links_pairs", "iv_links_select"], lambda: ctx.iv_links([rec_a, rec_b], 1), args.calls),
                                      links=int(links.size))
    per_iv, dist = ctx.edit_segments(g_a, g_b, iv, iv, segs, flip, BAND, with_distances=True)
    stepped = segs[(dist < EDIT_INVALID) | (dist == EDIT_OVERBAND)]              # (the segments whose whole band was stepped through)
    steps = int(stepped["dx"].astype(np.int64).sum() + stepped["dy"].astype(np.int64).sum())
    t = timed(ctx, ["edit_segments", "edit_reduce"], lambda: ctx.edit_segments(g_a, g_b, iv, iv, segs, flip, BAND), args.calls)
    cells = steps * (2 * BAND + 1) // 2
    out["edit_segments"] = dict(t, aligned_segments=int(per_iv["aligned"].sum()), aligned_bases_a=int(per_iv["aligned_a"].sum()), edits=int(per_iv["edits"].sum()),
                                overband=int(per_iv["overband"].sum()), invalid=int(per_iv["invalid"].sum()), antidiagonal_steps=steps, band_cells=cells,
                                band_cells_per_second=cells / (t["edit_segments"]["median_ms"] * 1e-3))
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

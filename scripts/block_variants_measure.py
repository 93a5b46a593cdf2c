#!/usr/bin/env python3
"""Device times of the block variants' call beside the block identity's (docs/design/04_17_block_variants.md) on two synthetic genomes
of one ancestor: `--bp` bases each at 1 % divergence, tiled by 10^4 intervals, interval i of one genome the mate of interval i of the
other, k 21, rate 16, band 31, max_len 4096 -- the pair of scripts/block_identity_measure.py.  One process, device events (the
library's timers), medians of six calls with minimum and maximum, a time limit.  The timers edit_segments, edit_script_plan and
edit_script on the same segments; ops and ops per second; the share of segments with D >= 1; the ratio edit_script / edit_segments.
Output: profiles/block_variants_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import EDIT_INVALID, Context, Genome  # noqa: E402
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
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_variants_measure.json"))
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
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)
    per_iv, dist = ctx.edit_segments(g_a, g_b, iv, iv, segs, flip, BAND, with_distances=True)      # warm-up, and the distances
    ops, first = ctx.edit_script(g_a, g_b, iv, iv, segs, flip, BAND, dist)
    assert ops.size == int(per_iv["edits"].sum()) == int(first[-1])
    aligned = dist < EDIT_INVALID
    t_seg = timed(ctx, ["edit_segments", "edit_reduce"], lambda: ctx.edit_segments(g_a, g_b, iv, iv, segs, flip, BAND), args.calls)
    t_scr = timed(ctx, ["edit_script_plan", "edit_script"], lambda: ctx.edit_script(g_a, g_b, iv, iv, segs, flip, BAND, dist), args.calls)
    out = {"bp": bp, "intervals": int(n_iv), "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "segments": int(segs.size),
           "aligned_segments": int(aligned.sum()), "segments_with_edits": int((aligned & (dist >= 1)).sum()),
           "share_with_edits": float((aligned & (dist >= 1)).sum()) / max(int(segs.size), 1), "ops": int(ops.size),
           "edit_segments": t_seg, "edit_script": t_scr,
           "ops_per_second": ops.size / (t_scr["edit_script"]["median_ms"] * 1e-3),
           "edit_script_over_edit_segments": t_scr["edit_script"]["median_ms"] / t_seg["edit_segments"]["median_ms"]}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

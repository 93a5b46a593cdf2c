#!/usr/bin/env python3
"""Device times of the edit scripts of the stretches beyond the band beside the wide pass that gives their distances
(docs/design/04_19_block_wide_variants.md), on the input and the parameters of scripts/block_identity_wide_measure.py: two genomes of
one ancestor made on the host, 1 % substitutions and one indel of 32 - 300 bases every `--every` bases, k 21, rate 16, band 31,
max_len 4096, E 1023.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit.
The timers edit_wide_script_plan and edit_wide_script, and edit_wide from the same call sequence on the same segments; ops per second,
the bytes of the tables and the number of batches at the default budget; the ratio edit_wide_script / edit_wide.
Output: profiles/block_wide_variants_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import EDIT_INVALID, SEG_OFFBAND, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_EDITS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_wide_variants_measure.json"))
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
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)
    _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)                            # warm-up, and the distances
    ops, first = ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final)
    plan = ctx.edit_wide_script_last_plan()
    gap = np.abs(segs["dy"].astype(np.int64) - segs["dx"].astype(np.int64))
    member = (final < EDIT_INVALID) & ((segs["kind"] == SEG_OFFBAND) | (final.astype(np.int64) + gap > 2 * BAND + 1))
    assert int(member.sum()) == plan["members"] and ops.size == int(final[member].sum()) == int(first[-1])

    def both():
        ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
        ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final)
    t = timed(ctx, ["edit_wide", "edit_wide_script_plan", "edit_wide_script"], both, args.calls)
    seconds = t["edit_wide_script"]["median_ms"] * 1e-3
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "segments": int(segs.size), "script_set": plan["members"], "script_set_offband": int((member & (segs["kind"] == SEG_OFFBAND)).sum()),
           "ops": int(ops.size), "mean_d": float(final[member].mean()) if member.any() else 0.0, "max_d": int(final[member].max()) if member.any() else 0,
           "ins_ops": int((ops["op"] == 3).sum()), "del_ops": int((ops["op"] == 2).sum()), "sub_ops": int((ops["op"] == 1).sum()),
           "table_bytes": plan["table_bytes"], "batches_at_default_budget": plan["batches"], "default_budget_bytes": 1 << 30,
           "times": t, "ops_per_second": ops.size / seconds, "members_per_second": plan["members"] / seconds,
           "edit_wide_script_over_edit_wide": t["edit_wide_script"]["median_ms"] / t["edit_wide"]["median_ms"]}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

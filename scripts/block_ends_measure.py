#!/usr/bin/env python3
"""Device time of the free-end extension behind the block identity (docs/design/04_20_block_ends.md) on the measurement input of
docs/design/04_18_block_identity_wide.md (scripts/block_identity_wide_measure.py `family`): two genomes of one ancestor made on the
host, `--bp` bases in `--intervals` paired tiles, 1 % substitutions and one indel of 32 - 300 bases every `--every` bases; k 21, rate 16,
band 31, max_len 4096, E 1023 for the identity pass, ends_max_len 4096, ends_max_edits 255, ends_penalty 6 for the extension.  Both
flanks of every tile with an aligned segment are one task each; a flank runs on into the neighbouring tile, which is collinear here.
One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit.  The timer edit_extend,
tasks per second, the split of the stop reasons, the bases and edits of the extensions; beside it edit_segments and edit_wide of the
same call as the point of comparison.  Output: profiles/block_ends_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd import assess  # noqa: E402
from ntsynt_amd.device import Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_EDITS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_ends_measure.json"))
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
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)          # warm-up, and the distances
    _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
    tasks, _ = assess.ends_tasks(segs, final, iv_a, iv_b, flip, [(i, i, i) for i in range(n_iv)], g_a.rec_len, g_b.rec_len, cap)
    results = ctx.edit_extend(g_a, g_b, tasks, penalty, limit)                                      # warm-up, and the results
    stops = Counter(assess.ends_stop(t, r, cap, limit) for t, r in zip(tasks, results))
    t_seg = timed(ctx, ["edit_segments"], lambda: ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True), args.calls)
    t_wide = timed(ctx, ["edit_wide"], lambda: ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist), args.calls)
    t_ext = timed(ctx, ["edit_extend"], lambda: ctx.edit_extend(g_a, g_b, tasks, penalty, limit), args.calls)
    seconds = t_ext["edit_extend"]["median_ms"] * 1e-3
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "ends_max_len": cap, "ends_max_edits": limit, "ends_penalty": penalty, "segments": int(segs.size), "tasks": int(tasks.size),
           "stop_reasons": dict(sorted(stops.items())), "extended_bases_a": int(results["ext_a"].sum()), "extended_bases_b": int(results["ext_b"].sum()),
           "extension_edits": int(results["edits"].sum()), "mean_rows_per_task": float(results["edits"].mean()) if tasks.size else 0.0,
           "edit_extend": t_ext, "edit_segments": t_seg, "edit_wide": t_wide, "tasks_per_second": tasks.size / seconds if seconds else None,
           "edit_extend_over_edit_segments": t_ext["edit_extend"]["median_ms"] / t_seg["edit_segments"]["median_ms"],
           "edit_extend_over_edit_wide": t_ext["edit_extend"]["median_ms"] / t_wide["edit_wide"]["median_ms"]}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

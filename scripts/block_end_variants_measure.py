#!/usr/bin/env python3
"""Device time of the edit scripts of the extended flanks (docs/design/04_21_block_end_variants.md) on the measurement input of
docs/design/04_20_block_ends.md (scripts/block_ends_measure.py): two genomes of one ancestor made on the host, `--bp` bases in
`--intervals` paired tiles, 1 % substitutions and one indel of 32 - 300 bases every `--every` bases; k 21, rate 16, band 31, max_len
4096, E 1023 for the identity pass, ends_max_len 4096, ends_max_edits 255, ends_penalty 6 for the extension: 2 000 tasks, both flanks of
every tile.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit.  The
timers edit_extend, edit_extend_script_plan and edit_extend_script of one call sequence on the same tasks; ops per second, the members,
the bytes of the tables and the number of batches at the default budget; the ratio edit_extend_script / edit_extend.  Output:
profiles/block_end_variants_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys

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
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_end_variants_measure.json"))
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
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)
    _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
    tasks, _ = assess.ends_tasks(segs, final, iv_a, iv_b, flip, [(i, i, i) for i in range(n_iv)], g_a.rec_len, g_b.rec_len, cap)
    results = ctx.edit_extend(g_a, g_b, tasks, penalty, limit)                                      # warm-up, and the results
    ops, first = ctx.edit_extend_script(g_a, g_b, tasks, results)                                   # warm-up, and the plan
    plan = ctx.edit_extend_script_last_plan()
    assert ops.size == int(results["edits"].sum()) == int(first[-1])

    def both():
        ctx.edit_extend(g_a, g_b, tasks, penalty, limit)
        ctx.edit_extend_script(g_a, g_b, tasks, results)
    t = timed(ctx, ["edit_extend", "edit_extend_script_plan", "edit_extend_script"], both, args.calls)
    seconds = t["edit_extend_script"]["median_ms"] * 1e-3
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "ends_max_len": cap, "ends_max_edits": limit, "ends_penalty": penalty, "tasks": int(tasks.size), "ops": int(ops.size),
           "largest_edits": int(results["edits"].max()) if tasks.size else 0, "extended_bases_a": int(results["ext_a"].sum()),
           "extended_bases_b": int(results["ext_b"].sum()), "members": plan["members"], "table_bytes": plan["table_bytes"], "batches": plan["batches"],
           "ops_per_second": ops.size / seconds if seconds else None}
    out.update(t)
    out["edit_extend_script_over_edit_extend"] = t["edit_extend_script"]["median_ms"] / t["edit_extend"]["median_ms"]
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

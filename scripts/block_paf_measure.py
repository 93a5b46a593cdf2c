#!/usr/bin/env python3
"""Device time of the CIGAR pass of the block alignments (docs/design/04_22_block_alignments.md) against the script calls that feed it, on
the measurement input of docs/design/04_20_block_ends.md (scripts/block_ends_measure.py): two genomes of one ancestor made on the host,
`--bp` bases in `--intervals` paired tiles, 1 % substitutions and one indel of 32 - 300 bases every `--every` bases; k 21, rate 16, band
31, max_len 4096, E 1023, ends_max_len 4096, ends_max_edits 255, ends_penalty 6.  One round holds all tiles: the pieces and ops are what
assess.block_alignments hands to nts_cigar_build.  One process, device events (the library's timers), medians of six calls with minimum
and maximum, a time limit.  The timers edit_script, edit_wide_script, edit_extend_script (and their plans) and cigar_atoms, cigar_merge of
one call sequence, each as ms per call (the per-scope median times the scopes per call: cigar_merge is opened twice); pieces, ops,
atoms, chains and entries; the ratio (cigar_atoms + cigar_merge) / (the script calls).  Output:
profiles/block_paf_measure.json.  Needs the GPU: there is no fallback."""
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

SCRIPT_TIMERS = ["edit_script_plan", "edit_script", "edit_wide_script_plan", "edit_wide_script", "edit_extend_script_plan", "edit_extend_script"]
CIGAR_TIMERS = ["cigar_atoms", "cigar_merge"]


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_paf_measure.json"))
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

    def scripts():
        return (ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist), ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final),
                ctx.edit_extend_script(g_a, g_b, tasks, results))
    narrow, wide, flank_script = scripts()                                                          # warm-up, and the ops
    pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
    ops, first = assess.alignment_ops(source, [narrow, wide], flank_script)
    n_chains = int(chains["line"].size)
    cigar, records = ctx.cigar_build(pieces, ops, first, n_chains)                                  # warm-up, and the entries
    assert int(records["n_cig"].sum()) == cigar.size and int(records["x"].sum() + records["ins"].sum() + records["del"].sum()) == ops.size

    def both():
        scripts()
        ctx.cigar_build(pieces, ops, first, n_chains)
    t = timed(ctx, SCRIPT_TIMERS + CIGAR_TIMERS, both, args.calls)

    def per_call(name):
        "`timed` gives ms per timed scope: a timer that is opened several times in one call (cigar_merge: twice) counts that often"
        scopes = t[name]["timed_launches_per_call"]
        assert len(scopes) == 1, (name, scopes)
        return t[name]["median_ms"] * scopes[0]
    per_call_ms = {name: per_call(name) for name in SCRIPT_TIMERS + CIGAR_TIMERS}
    script_ms = sum(per_call_ms[name] for name in SCRIPT_TIMERS)
    cigar_ms = sum(per_call_ms[name] for name in CIGAR_TIMERS)
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "ends_max_len": cap, "ends_max_edits": limit, "ends_penalty": penalty, "segments": int(segs.size), "pieces": int(pieces.size), "ops": int(ops.size),
           "atoms": int(2 * ops.size + pieces.size), "chains": n_chains, "entries": int(cigar.size), "aligned_bases_a": int(records["len_a"].sum()),
           "per_call_ms": per_call_ms, "script_calls_per_call_ms": script_ms, "cigar_per_call_ms": cigar_ms,
           "cigar_over_script_calls": cigar_ms / script_ms if script_ms else None}
    out.update(t)
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

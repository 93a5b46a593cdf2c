#!/usr/bin/env python3
"""Device time of the aligned rows of `--block-maf` (docs/design/04_29_block_maf.md) on the measurement input of
docs/design/04_22_block_alignments.md: two genomes of `--bp` bases, `--intervals` pairs, an indel every `--every` bases, at E = 0 without
ends and at E = 1023 with ends.  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time
limit: cigar_rows_scan and cigar_rows_emit of nts_cigar_rows beside cigar_merge of the nts_cigar_build that made the entries and
cigar_text_scan and cigar_text_emit of nts_cigar_text, in the same calls; the stored bytes per second of the emit kernel (both rows); and
the host clock of one whole cigar_rows call with its copies against a NumPy rendering of the same rows (assess.maf_rows_host over the
host copies of the genomes, one call per chain), the bytes compared.  Output: profiles/block_maf_measure.json.  Needs the GPU: there is
no fallback."""
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
from ntsynt_amd.device import Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_EDITS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402

TIMERS = ["cigar_merge", "cigar_text_scan", "cigar_text_emit", "cigar_rows_scan", "cigar_rows_emit"]
Round = type("Round", (), {})                                 # what alignment_spans reads of a _Round: iv_a, iv_b, flip, lines


def numpy_rows(cigar, records, spans, seq_a, seq_b):
    "both row buffers on the host: assess.maf_rows_host per chain over slices of the genomes (every chain of this input is forwards)"
    rows_a, rows_b = [], []
    for rec, sp in zip(records, spans):
        first, pa, pb = int(rec["first"]), int(sp["pos_a"]), int(sp["pos_b"])
        a, b = assess.maf_rows_host(cigar[first:first + int(rec["n_cig"])], seq_a[pa:pa + int(rec["len_a"])], seq_b[pb:pb + int(rec["len_b"])])
        rows_a.append(a)
        rows_b.append(b)
    return np.concatenate(rows_a), np.concatenate(rows_b)


def measure(ctx, g_a, g_b, seq_a, seq_b, iv_a, iv_b, wide, calls):
    cap, limit, penalty = assess.ENDS_MAX_LEN, assess.ENDS_MAX_EDITS, assess.ENDS_PENALTY
    n_iv = iv_a.shape[0]
    rec_a, _ = g_a.sample_intervals(iv_a, K, RATE)
    rec_b, _ = g_b.sample_intervals(iv_b, K, RATE)
    mate = np.arange(n_iv, dtype=np.uint32)
    len_b = (iv_b[:, 2] - iv_b[:, 1]).astype(np.uint32)
    flip = np.zeros(n_iv, dtype=np.uint8)
    lines = [(i, i, i) for i in range(n_iv)]
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, mate, len_b, flip, K, BAND, MAX_LEN)
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)
    scripts, final, flanks, results, flank_script = [ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist)], dist, None, None, None
    if wide:
        _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
        tasks, flanks = assess.ends_tasks(segs, final, iv_a, iv_b, flip, lines, g_a.rec_len, g_b.rec_len, cap)
        results = ctx.edit_extend(g_a, g_b, tasks, penalty, limit)
        scripts.append(ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final))
        flank_script = ctx.edit_extend_script(g_a, g_b, tasks, results)
    pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
    ops, first = assess.alignment_ops(source, scripts, flank_script)
    n_chains = int(chains["line"].size)
    cigar, records = ctx.cigar_build(pieces, ops, first, n_chains)
    rnd = Round()
    rnd.iv_a, rnd.iv_b, rnd.flip, rnd.lines = iv_a, iv_b, flip, lines
    spans = assess.alignment_spans(rnd, chains, flanks, results)
    _, _, cs, _ = ctx.cigar_text(cigar, records, spans, g_a, g_b)
    row_a, row_b, row_first = ctx.cigar_rows(cigar, records, spans, g_a, g_b)                 # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want_a, want_b = numpy_rows(cigar, records, spans, seq_a, seq_b)
        host.append((time.perf_counter() - t0) * 1e3)
    assert want_a.tobytes() == row_a.tobytes() and want_b.tobytes() == row_b.tobytes()
    columns = records["eq"] + records["x"] + records["ins"] + records["del"]
    assert np.array_equal(np.diff(row_first.astype(np.int64)), columns.astype(np.int64)) and set(np.unique(row_a).tolist()) <= set(b"ACGTN-")

    def all_three():
        ctx.cigar_build(pieces, ops, first, n_chains)
        ctx.cigar_text(cigar, records, spans, g_a, g_b)
        ctx.cigar_rows(cigar, records, spans, g_a, g_b)
    t = timed(ctx, TIMERS, all_three, calls)
    per_call_ms = {}
    for timer in TIMERS:
        scopes = t[timer]["timed_launches_per_call"]
        assert len(scopes) == 1, (timer, scopes)
        per_call_ms[timer] = {f: t[timer][f + "_ms"] * scopes[0] for f in ("median", "min", "max")}
    whole = []
    for _ in range(calls):
        t0 = time.perf_counter()
        ctx.cigar_rows(cigar, records, spans, g_a, g_b)
        whole.append((time.perf_counter() - t0) * 1e3)
    emit = per_call_ms["cigar_rows_emit"]["median"]
    return {"max_edits": MAX_EDITS if wide else 0, "ends": bool(wide), "chains": n_chains, "entries": int(cigar.size), "columns": int(row_a.size),
            "row_bytes": 2 * int(row_a.size), "cs_bytes": int(cs.size), "calls": calls, "timers": t, "per_call_ms": per_call_ms,
            "emit_stored_gb_per_s": 2 * int(row_a.size) / (emit * 1e-3) / 1e9 if emit else None,
            "rows_over_text_emit": emit / per_call_ms["cigar_text_emit"]["median"] if per_call_ms["cigar_text_emit"]["median"] else None,
            "host_cigar_rows_call_ms": {"median": statistics.median(whole), "min": min(whole), "max": max(whole)},
            "host_numpy_rows_ms": {"median": statistics.median(host), "min": min(host), "max": max(host)},
            "numpy_over_call": statistics.median(host) / statistics.median(whole)}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=540)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_maf_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    seq_a, seq_b, iv_a, iv_b = family(bp, args.intervals, args.every, np.random.default_rng(SEED))
    ctx = Context(0)
    ctx.profile(True)
    zero = np.zeros(1, dtype=np.uint64)
    g_a = Genome(ctx, ["a"], seq_a, zero, np.array([seq_a.size], dtype=np.uint64))
    g_b = Genome(ctx, ["b"], seq_b, zero, np.array([seq_b.size], dtype=np.uint64))
    out = {"bp": bp, "intervals": int(iv_a.shape[0]), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN,
           "shape": "one lane per 4-byte word of both rows (the wider lane was not tried)",
           "narrow": measure(ctx, g_a, g_b, seq_a, seq_b, iv_a, iv_b, False, args.calls),
           "wide_with_ends": measure(ctx, g_a, g_b, seq_a, seq_b, iv_a, iv_b, True, args.calls)}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: ({f: v[f] for f in ("chains", "entries", "columns", "per_call_ms", "emit_stored_gb_per_s", "host_cigar_rows_call_ms", "host_numpy_rows_ms")}
                          if isinstance(v, dict) else v) for k, v in out.items()}))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

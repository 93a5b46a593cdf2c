#!/usr/bin/env python3
"""Device time of the two tag texts of `--block-paf --paf-cs` (docs/design/04_26_block_paf_cs.md) on the measurement input of
docs/design/04_22_block_alignments.md: two genomes of `--bp` bases, `--intervals` pairs, an indel every `--every` bases.  One process,
device events (the library's timers), medians of six calls with minimum and maximum, a time limit: cigar_text_scan and cigar_text_emit of
nts_cigar_text (both texts) beside cigar_atoms and cigar_merge of the nts_cigar_build that made the entries, in the same calls; the
entries, chains and bytes of both texts; and the host clock of assess.cigar_texts on the same entries -- the parent's way to the cg
text -- and of one whole cigar_text call with its copies.  The device texts are checked against cigar_texts and, per chain, against the
lengths the records imply.  Output: profiles/block_paf_cs_measure.json.  Needs the GPU: there is no fallback."""
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

BUILD_TIMERS = ["cigar_atoms", "cigar_merge"]
TEXT_TIMERS = ["cigar_text_scan", "cigar_text_emit"]
Round = type("Round", (), {})                                 # what alignment_spans reads of a _Round: iv_a, iv_b, flip, lines


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_paf_cs_measure.json"))
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
    rnd = Round()
    rnd.iv_a, rnd.iv_b, rnd.flip, rnd.lines = iv_a, iv_b, flip, lines
    spans = assess.alignment_spans(rnd, chains, flanks, results)
    cg, cg_first, cs, cs_first = ctx.cigar_text(cigar, records, spans, g_a, g_b)               # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        texts = assess.cigar_texts(cigar, records["first"], records["n_cig"])
        host.append((time.perf_counter() - t0) * 1e3)
    assert "".join(texts).encode() == cg.tobytes() and [len(t) for t in texts] == np.diff(cg_first.astype(np.int64)).tolist()
    code, length = cigar & np.uint64(15), (cigar >> np.uint64(4)).astype(np.int64)
    assert int(cs.size) == int((np.char.str_len(length[code == 7].astype("S20")) + 1).sum() + 3 * length[code == 8].sum() + (length[(code == 1) | (code == 2)] + 1).sum())
    assert set(np.unique(cs).tolist()) <= set(b":*-+0123456789acgtn")

    def both():
        ctx.cigar_build(pieces, ops, first, n_chains)
        ctx.cigar_text(cigar, records, spans, g_a, g_b)
    t = timed(ctx, BUILD_TIMERS + TEXT_TIMERS, both, args.calls)
    per_call_ms = {}
    for timer in BUILD_TIMERS + TEXT_TIMERS:
        scopes = t[timer]["timed_launches_per_call"]
        assert len(scopes) == 1, (timer, scopes)
        per_call_ms[timer] = {f: t[timer][f + "_ms"] * scopes[0] for f in ("median", "min", "max")}
    whole = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ctx.cigar_text(cigar, records, spans, g_a, g_b)
        whole.append((time.perf_counter() - t0) * 1e3)
    build_ms = sum(per_call_ms[timer]["median"] for timer in BUILD_TIMERS)
    text_ms = sum(per_call_ms[timer]["median"] for timer in TEXT_TIMERS)
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "max_edits": MAX_EDITS,
           "ends_max_len": cap, "ends_max_edits": limit, "ends_penalty": penalty, "chains": n_chains, "entries": int(cigar.size),
           "entries_per_chain_max": int(records["n_cig"].max()), "aligned_bases_a": int(records["len_a"].sum()), "cg_bytes": int(cg.size),
           "cs_bytes": int(cs.size), "calls": args.calls, "timers": t, "per_call_ms": per_call_ms, "build_per_call_ms": build_ms, "text_per_call_ms": text_ms,
           "text_over_build": text_ms / build_ms if build_ms else None,
           "emit_over_merge": per_call_ms["cigar_text_emit"]["median"] / per_call_ms["cigar_merge"]["median"] if per_call_ms["cigar_merge"]["median"] else None,
           "host_cigar_texts_ms": {"median": statistics.median(host), "min": min(host), "max": max(host)},
           "host_cigar_text_call_ms": {"median": statistics.median(whole), "min": min(whole), "max": max(whole)}}
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the chain file's blocks and text (docs/design/04_28_block_chain.md) on the measurement input of
docs/design/04_22_block_alignments.md -- two genomes of `--bp` bases, `--intervals` pairs -- run twice: with E = 0 and without ends, so
that the chains of a pair break at the indels wider than the band (several chains per pair), and with E = 1023 and ends (one chain per
pair).  One process, device events (the library's timers), medians of six calls with minimum and maximum, a time limit:
chain_blocks_scan, chain_blocks_emit and chain_text of nts_cigar_chain_blocks beside cigar_merge of nts_cigar_build and lift_pairs_scan
of nts_cigar_lift_pairs in the same calls; the numbers of blocks and text bytes; and on the host clock one whole call against a NumPy
rendering of the same lines from the block records.  Output: profiles/block_chain_measure.json.  Needs the GPU: there is no fallback."""
import argparse
import faulthandler
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd import assess  # noqa: E402
from ntsynt_amd.device import PAIR_RANGE_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_EDITS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.gap_links_measure import timed  # noqa: E402

CHAIN_TIMERS = ["chain_blocks_scan", "chain_blocks_emit", "chain_text"]
BESIDE_TIMERS = ["cigar_merge", "lift_pairs_scan"]


def numpy_lines(pairs, blocks):
    "the text of all data lines from the block records with array operations alone: what a host without the device call would do"
    last = np.zeros(blocks.size, dtype=bool)
    has = pairs["n_blocks"] > 0
    last[(pairs["first_block"][has] + pairs["n_blocks"][has] - 1).astype(np.int64)] = True
    size, dt, dq = (blocks[f].astype("S20") for f in ("size", "dt", "dq"))
    full = np.char.add(np.char.add(np.char.add(np.char.add(size, b"\t"), dt), b"\t"), np.char.add(dq, b"\n"))
    return np.where(last, np.char.add(size, b"\n"), full).tobytes().replace(b"\0", b"")


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=500)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_chain_measure.json"))
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
    narrow = ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist)
    out = {"bp": bp, "intervals": int(n_iv), "indel_every": args.every, "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN, "calls": args.calls}
    for name in ("narrow_no_ends", "wide_with_ends"):
        if name == "narrow_no_ends":                          # E = 0: the narrow band alone, no flanks
            pieces, source, chains = assess.alignment_pieces(segs, dist, lines)
            ops, first = assess.alignment_ops(source, [narrow])
        else:                                                 # E = 1023 and ends
            _, final = ctx.edit_wide(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, dist)
            tasks, flanks = assess.ends_tasks(segs, final, iv_a, iv_b, flip, lines, g_a.rec_len, g_b.rec_len, cap)
            results = ctx.edit_extend(g_a, g_b, tasks, penalty, limit)
            wide, flank_script = ctx.edit_wide_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, MAX_EDITS, final), ctx.edit_extend_script(g_a, g_b, tasks, results)
            pieces, source, chains = assess.alignment_pieces(segs, final, lines, flanks, results)
            ops, first = assess.alignment_ops(source, [narrow, wide], flank_script)
        n_chains = int(chains["line"].size)
        cigar, records = ctx.cigar_build(pieces, ops, first, n_chains)
        links, pair_first, _, _ = assess.chain_links(assess._AlignmentRound(SimpleNamespace(lines=lines), None, None, None, chains, cigar, records))
        pair_first = pair_first.astype(np.uint64)
        no_range = np.zeros(0, dtype=PAIR_RANGE_DTYPE)
        pairs, blocks, text, text_first = ctx.cigar_chain_blocks(cigar, records, links, pair_first)     # warm-up, and the results
        t0 = time.perf_counter()
        ctx.cigar_chain_blocks(cigar, records, links, pair_first)
        call_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rendered = numpy_lines(pairs, blocks)
        numpy_ms = (time.perf_counter() - t0) * 1e3
        assert rendered == text.tobytes()

        def calls():
            ctx.cigar_build(pieces, ops, first, n_chains)
            ctx.cigar_lift_pairs(cigar, records, links, pair_first, no_range)
            ctx.cigar_chain_blocks(cigar, records, links, pair_first)
        t = timed(ctx, CHAIN_TIMERS + BESIDE_TIMERS, calls, args.calls)
        per_call_ms = {}
        for timer in CHAIN_TIMERS + BESIDE_TIMERS:            # (`timed` gives ms per timed scope: cigar_merge and chain_text are opened twice per call)
            scopes = t[timer]["timed_launches_per_call"]
            assert len(scopes) == 1, (timer, scopes)
            per_call_ms[timer] = {f: t[timer][f + "_ms"] * scopes[0] for f in ("median", "min", "max")}
        per_pair = np.diff(pair_first.astype(np.int64))
        out[name] = dict(t, max_edits=0 if name == "narrow_no_ends" else MAX_EDITS, ends=None if name == "narrow_no_ends" else [cap, limit, penalty],
                         chains=n_chains, links=int(links.size), entries=int(cigar.size), blocks=int(blocks.size), text_bytes=int(text.size),
                         liftover_chains=int(np.count_nonzero(pairs["n_blocks"])),
                         chains_per_pair={"min": int(per_pair.min()), "median": float(np.median(per_pair)), "max": int(per_pair.max())},
                         per_call_ms=per_call_ms, host_clock_ms={"cigar_chain_blocks_one_call": call_ms, "numpy_rendering_of_the_lines": numpy_ms})
    g_a.free()
    g_b.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

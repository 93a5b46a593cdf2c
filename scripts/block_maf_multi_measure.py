#!/usr/bin/env python3
"""Device time of the star merge of `--block-maf-multi` (docs/design/04_30_block_maf_multi.md) on the measurement input of
docs/design/04_22_block_alignments.md grown to three genomes: a reference of `--bp` bases and two queries derived from it with indels
`--every` and `--every` + 700 bases apart, `--intervals` blocks, at E = 0 without ends.  One process, device events (the library's
timers, summed per call: cigar_pad_sites is opened up to three times and cigar_pad_emit twice in one nts_cigar_pad), medians of six
calls with minimum and maximum, a time limit; the host clock of the whole pass (one cigar_pad, two cigar_rows(padded=True)) and of a
NumPy rendering of the same rows (assess.padded_rows_host per chain), the bytes compared.  Output:
profiles/block_maf_multi_measure.json.  Needs the GPU: there is no fallback."""
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
from ntsynt_amd.device import CHAIN_DTYPE, CIG_PAD_AT_DTYPE, CIG_SPAN_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_LEN, RATE, SEED, family  # noqa: E402

TIMERS = ["cigar_pad_sites", "cigar_pad_emit", "cigar_rows_scan", "cigar_rows_emit"]
Round = type("Round", (), {})                                 # what alignment_spans reads of a _Round: iv_a, iv_b, flip, lines


def cores_of(ctx, g_a, g_b, iv_a, iv_b):
    "the core chains of one star pair at E = 0 without ends: (entries per chain, group, t0, len_a, len_b, pos_b)"
    n_iv = iv_a.shape[0]
    rec_a, _ = g_a.sample_intervals(iv_a, K, RATE)
    rec_b, _ = g_b.sample_intervals(iv_b, K, RATE)
    flip = np.zeros(n_iv, dtype=np.uint8)
    lines = [(i, i, i) for i in range(n_iv)]
    segs, _ = ctx.iv_anchor_segments(rec_a, rec_b, np.arange(n_iv, dtype=np.uint32), (iv_b[:, 2] - iv_b[:, 1]).astype(np.uint32), flip, K, BAND, MAX_LEN)
    _, dist = ctx.edit_segments(g_a, g_b, iv_a, iv_b, segs, flip, BAND, with_distances=True)
    pieces, source, chains = assess.alignment_pieces(segs, dist, lines, None, None)
    ops, first = assess.alignment_ops(source, [ctx.edit_script(g_a, g_b, iv_a, iv_b, segs, flip, BAND, dist)], None)
    cigar, records = ctx.cigar_build(pieces, ops, first, int(chains["line"].size))
    rnd = Round()
    rnd.iv_a, rnd.iv_b, rnd.flip, rnd.lines = iv_a, iv_b, flip, lines
    spans = assess.alignment_spans(rnd, chains, None, None)
    first, n_cig, len_a, len_b, pos_a, pos_b = assess.chain_cores(cigar, records, spans)
    keep = np.flatnonzero(n_cig > 0)
    return [(int(chains["line"][c]), int(pos_a[c]), cigar[first[c]:first[c] + n_cig[c]], int(len_a[c]), int(len_b[c]), int(pos_b[c])) for c in keep.tolist()]


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=540)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_maf_multi_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    seq_a, seq_b, iv_a, iv_b = family(bp, args.intervals, args.every, np.random.default_rng(SEED))
    again, seq_c, _, iv_c = family(bp, args.intervals, args.every + 700, np.random.default_rng(SEED))
    assert np.array_equal(seq_a, again), "the third genome must derive from the same reference"
    ctx = Context(0)
    ctx.profile(True)
    zero = np.zeros(1, dtype=np.uint64)
    genomes = [Genome(ctx, [n], s, zero, np.array([s.size], dtype=np.uint64)) for n, s in (("a", seq_a), ("b", seq_b), ("c", seq_c))]
    held = []                                                 # (group, row, t0, entries, len_a, len_b, pos_b)
    for row, (g, iv) in enumerate(((genomes[1], iv_b), (genomes[2], iv_c)), 1):
        held += [(c[0], row) + c[1:] for c in cores_of(ctx, genomes[0], g, iv_a, iv)]
    held.sort(key=lambda h: h[:3])
    entries = np.concatenate([h[3] for h in held]).astype(np.uint64)
    records = np.zeros(len(held), dtype=CHAIN_DTYPE)
    records["n_cig"] = [h[3].size for h in held]
    records["first"] = np.concatenate(([0], np.cumsum(records["n_cig"][:-1].astype(np.int64))))
    records["len_a"], records["len_b"] = [h[4] for h in held], [h[5] for h in held]
    at = np.zeros(len(held), dtype=CIG_PAD_AT_DTYPE)
    at["group"], at["t0"] = [h[0] for h in held], [h[2] for h in held]
    members = {row: [j for j, h in enumerate(held) if h[1] == row] for row in (1, 2)}

    def whole_pass():
        padded, pad_first, _, site_pos, _ = ctx.cigar_pad(entries, records, at, int(iv_a.shape[0]))
        pad_first = pad_first.astype(np.int64)
        out = {}
        for row, mine in members.items():
            sub = np.zeros(len(mine), dtype=CHAIN_DTYPE)
            sub["n_cig"] = (pad_first[1:] - pad_first[:-1])[mine]
            sub["first"] = np.concatenate(([0], np.cumsum(sub["n_cig"][:-1].astype(np.int64))))
            sub["len_a"], sub["len_b"] = records["len_a"][mine], records["len_b"][mine]
            spans = np.zeros(len(mine), dtype=CIG_SPAN_DTYPE)
            spans["pos_a"], spans["pos_b"] = [held[j][2] for j in mine], [held[j][6] for j in mine]
            cigar = np.concatenate([padded[pad_first[j]:pad_first[j + 1]] for j in mine])
            out[row] = ctx.cigar_rows(cigar, sub, spans, genomes[0], genomes[row], padded=True)
        return padded, pad_first, site_pos, out

    padded, pad_first, site_pos, rows = whole_pass()          # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = {}
        for row, mine in members.items():
            seq = (seq_b, seq_c)[row - 1]
            made = [assess.padded_rows_host(padded[pad_first[j]:pad_first[j + 1]], seq_a[held[j][2]:held[j][2] + held[j][4]],
                                            seq[held[j][6]:held[j][6] + held[j][5]]) for j in mine]
            want[row] = ("".join(m[0] for m in made), "".join(m[1] for m in made))
        host.append((time.perf_counter() - t0) * 1e3)
    for row in members:
        assert want[row] == (rows[row][0].tobytes().decode(), rows[row][1].tobytes().decode()), row
    per_call, clock = {t: [] for t in TIMERS}, []
    for _ in range(args.calls):
        before = {t: ctx.timing(t)[0] for t in TIMERS}
        t0 = time.perf_counter()
        whole_pass()
        clock.append((time.perf_counter() - t0) * 1e3)
        for t in TIMERS:
            per_call[t].append(ctx.timing(t)[0] - before[t])

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}
    out = {"bp": bp, "intervals": int(iv_a.shape[0]), "indel_every": [args.every, args.every + 700], "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN,
           "chains": len(held), "entries": int(entries.size), "padded_entries": int(padded.size), "sites": int(site_pos.size),
           "row_bytes": int(sum(2 * r[0].size for r in rows.values())), "calls": args.calls,
           "per_call_ms": {t: spread(per_call[t]) for t in TIMERS}, "host_whole_pass_ms": spread(clock), "host_numpy_rows_ms": spread(host)}
    for g in genomes:
        g.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

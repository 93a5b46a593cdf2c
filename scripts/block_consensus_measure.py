#!/usr/bin/env python3
"""Device time of nts_cigar_profile, the call behind `--block-consensus` (docs/design/04_33_block_consensus.md), by the method of
scripts/block_conservation_measure.py.  Input A is that of scripts/block_maf_multi_measure.py: a reference of `--bp` bases and two
queries derived from it with indels `--every` and `--every` + 700 bases apart, `--intervals` blocks, at E = 0 without ends; the core
chains of the two star pairs.  Input B is the same family with planted indels of 1 to 8 bases, which the 31-diagonal band aligns, so
that the chains hold insertions and deletions.  One process, device events (the library's timers, summed over a call's openings),
medians of six calls with minimum and maximum, a time limit; the host clock of the call and of the NumPy rendering of the same columns
(assess.profile_host per group) as the only baseline, the bytes compared, six calls compared.  Output:
profiles/block_consensus_measure.json.  Needs the GPU: there is no fallback."""
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
from ntsynt_amd.device import CIG_PAD_AT_DTYPE, CIG_PROFILE_COL_DTYPE, CIG_PROFILE_REF, CIG_SPAN_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, DIVERGENCE, K, LETTERS, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.block_maf_multi_measure import cores_of  # noqa: E402
from scripts.block_variant_sites_measure import records_of  # noqa: E402

TIMERS = ["cigar_profile_events", "cigar_profile_emit"]


def small_family(bp, tiles, every, rng):
    "scripts.block_identity_wide_measure.family with indels of 1 to 8 bases: the same reference for the same generator"
    a = LETTERS[rng.integers(0, 4, size=bp)]
    b = a.copy()
    hit = np.flatnonzero(rng.random(bp) < DIVERGENCE)
    b[hit] = LETTERS[(np.searchsorted(LETTERS, b[hit]) + rng.integers(1, 4, size=hit.size)) % 4]
    step = -(-bp // tiles)
    pieces, iv_a, iv_b, at_b = [], [], [], 0
    for s in range(0, bp, step):
        e, size, at = min(s + step, bp), 0, s
        for where in range(s + every // 2, e - 400, every):
            n = int(rng.integers(1, 9))
            pieces.append(b[at:where])
            size += where - at
            if rng.random() < 0.5:
                pieces.append(LETTERS[rng.integers(0, 4, size=n)])
                size += n
                at = where
            else:
                at = where + n
        pieces.append(b[at:e])
        size += e - at
        iv_a.append((0, s, e))
        iv_b.append((0, at_b, at_b + size))
        at_b += size
    return a, np.concatenate(pieces), np.array(iv_a, dtype=np.uint64), np.array(iv_b, dtype=np.uint64)


def host_profile(entries, records, at, ref, alt, ref_first, alt_first, n_groups):
    "the columns of every group by assess.profile_host, as nts_cigar_profile returns them"
    cut = np.searchsorted(at["group"], np.arange(n_groups + 1))
    parts, col_first = [], np.zeros(n_groups + 1, dtype=np.uint64)
    for g in range(n_groups):
        lo, hi = int(cut[g]), int(cut[g + 1])
        col_first[g + 1] = col_first[g]
        if hi == lo:
            continue
        e_lo, e_hi = int(records["first"][lo]), int(records["first"][hi - 1] + records["n_cig"][hi - 1])
        sub = records[lo:hi].copy()
        sub["first"] -= e_lo
        part = assess.profile_host(entries[e_lo:e_hi], sub, at[lo:hi], ref[int(ref_first[lo]):int(ref_first[hi])], alt[int(alt_first[lo]):int(alt_first[hi])])
        part["group"] = g
        parts.append(part)
        col_first[g + 1] += part.size
    return np.concatenate(parts) if parts else np.zeros(0, dtype=CIG_PROFILE_COL_DTYPE), col_first


def measure(ctx, make, bp, intervals, every, calls):
    "one input: the family made by `make`, its cores, the bytes, the call timed `calls` times and compared with the host's rendering"
    seq_a, seq_b, iv_a, iv_b = make(bp, intervals, every, np.random.default_rng(SEED))
    again, seq_c, _, iv_c = make(bp, intervals, every + 700, np.random.default_rng(SEED))
    assert np.array_equal(seq_a, again), "the third genome must derive from the same reference"
    zero = np.zeros(1, dtype=np.uint64)
    genomes = [Genome(ctx, [n], s, zero, np.array([s.size], dtype=np.uint64)) for n, s in (("a", seq_a), ("b", seq_b), ("c", seq_c))]
    pairs, held = [], []
    for row, (g, iv) in enumerate(((genomes[1], iv_b), (genomes[2], iv_c)), 1):
        cores = cores_of(ctx, genomes[0], g, iv_a, iv)
        pairs.append(cores)
        held += [(c[0], row, c[1], c[2], c[3], c[4], row - 1, q) for q, c in enumerate(cores)]
    held.sort(key=lambda h: h[:3])
    n_groups = int(iv_a.shape[0])
    per_pair = []
    for pair, cores in enumerate(pairs):
        entries, records = records_of(cores)
        spans = np.zeros(len(cores), dtype=CIG_SPAN_DTYPE)
        spans["pos_a"], spans["pos_b"] = [c[1] for c in cores], [c[5] for c in cores]
        per_pair.append(ctx.cigar_var_bases(entries, records, spans, genomes[0], genomes[1 + pair]))
    entries, records = records_of([(h[0], h[2], h[3], h[4], h[5], 0) for h in held])
    at = np.zeros(len(held), dtype=CIG_PAD_AT_DTYPE)
    at["group"], at["t0"] = [h[0] for h in held], [h[2] for h in held]
    refs = [per_pair[h[6]][0][int(per_pair[h[6]][1][h[7]]):int(per_pair[h[6]][1][h[7] + 1])] for h in held]
    alts = [per_pair[h[6]][2][int(per_pair[h[6]][3][h[7]]):int(per_pair[h[6]][3][h[7] + 1])] for h in held]
    ref, alt = np.concatenate(refs), np.concatenate(alts)
    ref_first, alt_first = (np.concatenate(([0], np.cumsum([x.size for x in xs]))) for xs in (refs, alts))
    cols, col_first = ctx.cigar_profile(entries, records, at, ref, alt, n_groups)                      # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = host_profile(entries, records, at, ref, alt, ref_first, alt_first, n_groups)
        host.append((time.perf_counter() - t0) * 1e3)
    assert cols.tobytes() == want[0].tobytes() and col_first.tobytes() == want[1].tobytes(), "the device's columns are not the host's"
    per_call, clock = {t: [] for t in TIMERS}, []
    for _ in range(calls):
        before = {t: ctx.timing(t)[0] for t in TIMERS}
        t0 = time.perf_counter()
        got = ctx.cigar_profile(entries, records, at, ref, alt, n_groups)
        clock.append((time.perf_counter() - t0) * 1e3)
        assert got[0].tobytes() == cols.tobytes() and got[1].tobytes() == col_first.tobytes(), "a repeated call gives other bytes"
        for t in TIMERS:
            per_call[t].append(ctx.timing(t)[0] - before[t])
    for g in genomes:
        g.free()

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}
    code, size = (entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64)
    slot = cols["sub"] != CIG_PROFILE_REF
    return {"chains": len(held), "entries": int(entries.size), "events": int(size[np.isin(code, (1, 2, 8))].sum()),
            "i_entries": int((code == 1).sum()), "d_entries": int((code == 2).sum()), "columns": int(cols.size), "insertion_columns": int(slot.sum()),
            "sites": int(np.unique(np.stack((cols["group"][slot].astype(np.int64), cols["pos"][slot].astype(np.int64)), axis=1), axis=0).shape[0]),
            "widest_slot": int(cols["sub"][slot].max()) + 1 if slot.any() else 0, "deepest_column": int(cols["aligned"].max()) if cols.size else 0,
            "changed_calls": int((cols["call"] != cols["ref"]).sum()), "ref_bytes": int(ref.size), "alt_bytes": int(alt.size),
            "per_call_ms": {t: spread(per_call[t]) for t in TIMERS}, "host_call_ms": spread(clock), "host_numpy_profile_ms": spread(host)}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=1100)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_consensus_measure.json"))
    args = p.parse_args()
    faulthandler.dump_traceback_later(args.limit_seconds, exit=True)
    bp = int(args.bp)
    ctx = Context(0)
    ctx.profile(True)
    out = {"bp": bp, "intervals": args.intervals, "indel_every": [args.every, args.every + 700], "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN,
           "calls": args.calls, "input_a": measure(ctx, family, bp, args.intervals, args.every, args.calls),
           "input_b_indels_of_1_to_8": measure(ctx, small_family, bp, args.intervals, args.every, args.calls)}
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of nts_cigar_var_bases and nts_cigar_alleles, the calls behind `--block-variant-sites`
(docs/design/04_32_block_variant_sites.md), on the input and by the method of scripts/block_maf_multi_measure.py: a reference of `--bp`
bases and two queries derived from it with indels `--every` and `--every` + 700 bases apart, `--intervals` blocks, at E = 0 without
ends; the core chains of the two star pairs.  One process, device events (the library's timers, summed over a call's openings), medians
of six calls with minimum and maximum, a time limit; the host clock of both calls and of the NumPy rendering of the same alleles
(assess.alleles_host per group) as the only baseline, the bytes compared.  nts_cigar_var_bases is timed on the first pair's chains
(the stage makes one such call per pair).  Output: profiles/block_variant_sites_measure.json.  Needs the GPU: there is no fallback."""
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
from ntsynt_amd.device import CHAIN_DTYPE, CIG_ALLELE_DTYPE, CIG_PAD_AT_DTYPE, CIG_SPAN_DTYPE, Context, Genome  # noqa: E402
from scripts.block_identity_wide_measure import BAND, K, MAX_LEN, RATE, SEED, family  # noqa: E402
from scripts.block_maf_multi_measure import cores_of  # noqa: E402

BASES = ["cigar_var_bases_scan", "cigar_var_bases_emit"]
ALLELES = ["cigar_alleles_events", "cigar_alleles_emit"]


def records_of(cores):
    "(entries, CHAIN records) of a list of cores (group, t0, entries, len_a, len_b, pos_b)"
    records = np.zeros(len(cores), dtype=CHAIN_DTYPE)
    records["n_cig"] = [c[2].size for c in cores]
    records["first"] = np.concatenate(([0], np.cumsum(records["n_cig"][:-1].astype(np.int64))))
    records["len_a"], records["len_b"] = [c[3] for c in cores], [c[4] for c in cores]
    return np.concatenate([c[2] for c in cores]).astype(np.uint64), records


def host_alleles(entries, records, at, alt, ref_first, alt_first, n_groups):
    "the alleles of every group by assess.alleles_host, as nts_cigar_alleles returns them"
    cut = np.searchsorted(at["group"], np.arange(n_groups + 1))
    parts, carriers, allele_first, n_car = [], [], np.zeros(n_groups + 1, dtype=np.uint64), 0
    for g in range(n_groups):
        lo, hi = int(cut[g]), int(cut[g + 1])
        allele_first[g + 1] = allele_first[g]
        if hi == lo:
            continue
        e_lo, e_hi = int(records["first"][lo]), int(records["first"][hi - 1] + records["n_cig"][hi - 1])
        sub = records[lo:hi].copy()
        sub["first"] -= e_lo
        pos, kind, size, ref_off, alt_off, n, mine = assess.alleles_host(entries[e_lo:e_hi], sub, at[lo:hi], alt[int(alt_first[lo]):int(alt_first[hi])])
        part = np.zeros(pos.size, dtype=CIG_ALLELE_DTYPE)
        part["pos"], part["len"], part["group"], part["kind"], part["n_carriers"] = pos, size, g, kind, n
        part["ref_off"], part["alt_off"] = np.where(kind == 3, 0, ref_off + int(ref_first[lo])), np.where(kind == 2, 0, alt_off + int(alt_first[lo]))
        part["carrier_first"] = n_car + np.cumsum(n) - n
        n_car += int(n.sum())
        parts.append(part)
        carriers.append(mine + lo)
        allele_first[g + 1] += pos.size
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=CIG_ALLELE_DTYPE), allele_first,
            np.concatenate(carriers).astype(np.uint32) if carriers else np.zeros(0, dtype=np.uint32))


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--bp", type=float, default=2e7)
    p.add_argument("--intervals", type=int, default=1000)
    p.add_argument("--every", type=int, default=2000)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--limit-seconds", type=int, default=540)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "block_variant_sites_measure.json"))
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
    pairs, held = [], []                                      # per pair its cores; all cores as (group, row, t0, entries, len_a, len_b, pair, index in pair)
    for row, (g, iv) in enumerate(((genomes[1], iv_b), (genomes[2], iv_c)), 1):
        cores = cores_of(ctx, genomes[0], g, iv_a, iv)
        pairs.append(cores)
        held += [(c[0], row, c[1], c[2], c[3], c[4], row - 1, q) for q, c in enumerate(cores)]
    held.sort(key=lambda h: h[:3])
    n_groups = int(iv_a.shape[0])

    def var_bases(pair):
        cores = pairs[pair]
        entries, records = records_of(cores)
        spans = np.zeros(len(cores), dtype=CIG_SPAN_DTYPE)
        spans["pos_a"], spans["pos_b"] = [c[1] for c in cores], [c[5] for c in cores]
        return ctx.cigar_var_bases(entries, records, spans, genomes[0], genomes[1 + pair])
    per_pair = [var_bases(0), var_bases(1)]                   # warm-up, and the bytes
    entries, records = records_of([(h[0], h[2], h[3], h[4], h[5], 0) for h in held])
    at = np.zeros(len(held), dtype=CIG_PAD_AT_DTYPE)
    at["group"], at["t0"] = [h[0] for h in held], [h[2] for h in held]
    refs = [per_pair[h[6]][0][int(per_pair[h[6]][1][h[7]]):int(per_pair[h[6]][1][h[7] + 1])] for h in held]
    alts = [per_pair[h[6]][2][int(per_pair[h[6]][3][h[7]]):int(per_pair[h[6]][3][h[7] + 1])] for h in held]
    ref, alt = np.concatenate(refs), np.concatenate(alts)
    ref_first, alt_first = (np.concatenate(([0], np.cumsum([x.size for x in xs]))) for xs in (refs, alts))
    alleles, allele_first, carriers = ctx.cigar_alleles(entries, records, at, alt, n_groups)          # warm-up, and the results
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = host_alleles(entries, records, at, alt, ref_first, alt_first, n_groups)
        host.append((time.perf_counter() - t0) * 1e3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((alleles, allele_first, carriers), want)), "the device's alleles are not the host's"
    per_call, clock = {t: [] for t in BASES + ALLELES}, {"cigar_var_bases": [], "cigar_alleles": []}
    for _ in range(args.calls):
        for name, timers, call, first in (("cigar_var_bases", BASES, lambda: var_bases(0), per_pair[0]),
                                          ("cigar_alleles", ALLELES, lambda: ctx.cigar_alleles(entries, records, at, alt, n_groups), (alleles, allele_first, carriers))):
            before = {t: ctx.timing(t)[0] for t in timers}
            t0 = time.perf_counter()
            got = call()
            clock[name].append((time.perf_counter() - t0) * 1e3)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, first)), name + ": a repeated call gives other bytes"
            for t in timers:
                per_call[t].append(ctx.timing(t)[0] - before[t])

    def spread(values):
        return {"median": statistics.median(values), "min": min(values), "max": max(values)}
    kinds = {name: int((alleles["kind"] == k).sum()) for k, name in assess.VARIANT_SITE_TYPES.items()}
    out = {"bp": bp, "intervals": n_groups, "indel_every": [args.every, args.every + 700], "k": K, "rate": RATE, "band": BAND, "max_len": MAX_LEN,
           "chains": len(held), "entries": int(entries.size), "events": int(carriers.size), "alleles": int(alleles.size), "alleles_by_kind": kinds,
           "shared_alleles": int((alleles["n_carriers"] > 1).sum()), "ref_bytes": int(ref.size), "alt_bytes": int(alt.size),
           "var_bases_chains": len(pairs[0]), "var_bases_bytes": [int(per_pair[0][0].size), int(per_pair[0][2].size)],
           "longest_insertion": int(alleles["len"][alleles["kind"] == 3].max()) if kinds["ins"] else 0,
           "calls": args.calls, "per_call_ms": {t: spread(per_call[t]) for t in BASES + ALLELES}, "host_call_ms": {n: spread(v) for n, v in clock.items()},
           "host_numpy_alleles_ms": spread(host)}
    for g in genomes:
        g.free()
    ctx.close()
    with open(args.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()

"""Measurement behind docs/design/04_9_gap_content.md "Measured": k_bf_count_intervals against the every-k-mer-probed sketch pass
(k_hash<MODE_KEYS>, sketch mode "dense" without the summary) on the same genome and the same filter in the same process.

    python scripts/gaps_measure.py [--bp 3000000000] [--launches 6] [--out FILE.json]

A 3 Gbp synthetic genome (24 contigs) cut into 10^4 tiling intervals, the common filter of the three-genome 1 % family; both kernels
are timed with device events (nts_timing) and the whole call with the host clock around it (the call ends in a stream
synchronisation).  Run it under `rocprofv3 --kernel-trace --stats -- python scripts/gaps_measure.py` for the kernel times of the
trace, in a run of its own.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import BloomFilter, Context, Genome, bf_size_bytes, sketch  # noqa: E402


def tiling(g, n):
    "n intervals of equal length that tile the records of g"
    per_rec = max(1, n // len(g.names))
    rows = []
    for rec, length in enumerate(int(x) for x in g.rec_len):
        step = -(-length // per_rec)
        rows += [(rec, a, min(a + step, length)) for a in range(0, length, step)]
    return np.array(rows, dtype=np.uint64)


def timed(ctx, name, fn, launches):
    """(median, min, max) ms per launch of timer `name` by device events, the host-clock ms of every call of fn, and the timed launches
    per call (the caller checks that it is the one launch it means to compare)"""
    per_launch, host, counted = [], [], set()
    for _ in range(launches):
        ms0, n0 = ctx.timing(name)
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        host.append((time.perf_counter() - t0) * 1e3)
        ms1, n1 = ctx.timing(name)
        per_launch.append((ms1 - ms0) / max(n1 - n0, 1))
        counted.add(int(n1 - n0))
    return {"median_ms": statistics.median(per_launch), "min_ms": min(per_launch), "max_ms": max(per_launch), "launches": launches,
            "host_ms_median": statistics.median(host), "timed_launches_per_call": sorted(counted)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bp", type=int, default=3_000_000_000)
    p.add_argument("--k", type=int, default=24)
    p.add_argument("--launches", type=int, default=6)
    p.add_argument("--intervals", type=int, default=10_000)
    p.add_argument("--out")
    args = p.parse_args()
    k = args.k
    ctx = Context(0)
    g = Genome.synth(ctx, args.bp, 24, 20240207, 1000, 0.005)
    _, nbytes = bf_size_bytes(g.total_bp, 0.025)
    bf = BloomFilter(ctx, nbytes, k)
    bf.insert(g)
    for j in (1, 2):                                            # the family's other two genomes, one resident at a time
        other = Genome.synth(ctx, args.bp, 24, 20240207, 1000 + j, 0.005)
        bf.insert_and(other)
        other.free()
    occupancy = bf.get_fpr()
    n_kmers = g.valid_kmers(k)
    out = {"bp": args.bp, "k": k, "filter_bytes": nbytes, "occupancy": occupancy, "valid_kmers": n_kmers}
    iv = tiling(g, args.intervals)
    ctx.profile(2)
    kmers, hits = g.bf_count_intervals(bf, iv, k)             # warm-up, and the figures themselves
    out["intervals"] = int(iv.shape[0])
    out["kmers_counted"], out["hits"] = int(kmers.sum()), int(hits.sum())
    out["bf_count_iv"] = timed(ctx, "bf_count_iv", lambda: g.bf_count_intervals(bf, iv, k), args.launches)
    # the yardstick: the sketch's every-k-mer-probed key pass over the same k-mers (it also writes 8 bytes per k-mer)
    ctx.sketch_mode("dense")
    ctx.sketch_summary("never")
    sketch(ctx, g, k, 1000, bf).free()
    out["hash_probe"] = timed(ctx, "hash_probe", lambda: sketch(ctx, g, k, 1000, bf).free(), args.launches)
    ctx.sketch_mode("auto")
    ctx.sketch_summary("auto")
    out["ratio_to_yardstick"] = out["bf_count_iv"]["median_ms"] / out["hash_probe"]["median_ms"]
    out["random_probe_ms"] = bf.bench_random_probe(n_kmers, repeats=3)
    out["ratio_to_random_probe"] = out["bf_count_iv"]["median_ms"] / out["random_probe_ms"]
    out["probes_per_s"] = n_kmers / (out["bf_count_iv"]["median_ms"] * 1e-3)
    # many short intervals: what a table of short gaps looks like to the kernel (small tiles leave lanes idle)
    short = tiling(g, 1_000_000)
    short[:, 2] = np.minimum(short[:, 2], short[:, 1] + 1000)   # 10^6 intervals of 1000 bases, spread over the genome
    ks, hs = g.bf_count_intervals(bf, short, k)
    out["short"] = dict(timed(ctx, "bf_count_iv", lambda: g.bf_count_intervals(bf, short, k), args.launches), intervals=int(short.shape[0]),
                        kmers=int(ks.sum()))
    out["short"]["probes_per_s"] = out["short"]["kmers"] / (out["short"]["median_ms"] * 1e-3)
    ctx.profile(False)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")
    # the comparison holds only if each sketch call timed exactly one k_hash<MODE_KEYS> launch under "hash_probe", and each count call one launch
    assert out["hash_probe"]["timed_launches_per_call"] == [1] and out["bf_count_iv"]["timed_launches_per_call"] == [1], out
    g.free()
    bf.free()
    ctx.close()


if __name__ == "__main__":
    main()

"""Measurement behind docs/design/04_10_gap_links.md "Measured": the two launches of nts_bf_sample_intervals (k_bf_sample<false> counts,
k_bf_sample<true> writes) against k_bf_count_intervals on the same genome, the same intervals and the same filter in the same process,
and nts_iv_links on three genomes' samples.  With --hset, the measurement behind docs/design/04_11_gap_block_links.md instead: hset_build for
the hashes of a tenth of the intervals' rate-16 samples, the two launches of nts_hset_sample_intervals over all intervals, and the two
launches of nts_bf_sample_intervals over the same intervals in the same process as the yardstick.  With --hcount, the measurement behind
docs/design/04_12_gap_copies.md: the counting sweep (nts_hset_count_intervals, timer hcount_sweep) over the whole genome against the same
set, beside k_hset_sample<false> (timer hset_sample_count) on the same tiles in the same process; nts_hcount_add of as many values as the
sweep had hits; the clear and the read-back of the set's counts; and the same sweep of an assembly-like genome (satellite arrays: many
adds to one address) beside that of the uniform one, each against the hashes of a tenth of its own rate-16 sample.  With --sites, the
measurement behind docs/design/04_13_gap_copy_sites.md: after one count sweep of the same tiles, the two launches of
nts_hset_sample_intervals_capped (timers hcount_sample_count / hcount_sample_write) at cap 16 and at cap 2^32 - 1 beside
k_hset_sample<false / true> on the same tiles in the same process -- the difference at cap 2^32 - 1 is the price of the dependent 4-byte
load per member hit, the difference between the two caps the stores saved --; and one nts_iv_sites call of three genomes' lists (the
rate-16 samples of a tenth of each genome's intervals) against the first genome's cap-16 occurrences, its three timers beside
nts_iv_links' on the same lists.  With --periods, the measurement behind docs/design/04_14_gap_periods.md: the two launches of
nts_sample_intervals (timers iv_sample_count / iv_sample_write) beside k_bf_sample<false / true> on the same tiles in the same process
-- the sampler that probes nothing does strictly less per k-mer --, and one nts_iv_periods call on the records of a tenth of the
intervals, its three timers (--sites times nts_iv_sites on lists of that size from the same input).  With --families, the measurement
behind docs/design/04_15_gap_families.md: on the unfiltered rate-16 records of a tenth of the intervals, nts_iv_period_hashes (timer
iv_phash) with the periods nts_iv_periods finds on them, nts_iv_families (iv_families_join) with those records as pairs, and
nts_iv_family_sites (iv_family_sites_label / iv_family_sites_select) on the whole genome's occurrences of their hashes, beside the
parent's nts_iv_periods on the same records and nts_iv_sites of those records against as many occurrences, the yardsticks.

    python scripts/gap_links_measure.py [--bp 3000000000] [--calls 6] [--out FILE.json] [--hset | --hcount | --sites | --periods | --families]

A 3 Gbp synthetic genome (24 contigs) cut into 10^4 tiling intervals, the common filter of the three-genome 1 % family.  The launches
are timed with device events (nts_timing), the whole call with the host clock around it.  Rate 1 writes a record for every k-mer the
filter holds -- 16 bytes each, copied to the host --, so it is taken over the first tenth of the intervals.  Run it under
`rocprofv3 --kernel-trace --stats -- python scripts/gap_links_measure.py` for the kernel times of the trace, in a run of its own.
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

from ntsynt_amd.device import BloomFilter, Context, Genome, HashCounts, HashSet, bf_size_bytes  # noqa: E402

SEED, DIVERGENCE = 20240207, 0.005                              # scripts/gaps_measure.py's family


def tiling(g, n):
    "n intervals of equal length that tile the records of g"
    per_rec = max(1, n // len(g.names))
    rows = []
    for rec, length in enumerate(int(x) for x in g.rec_len):
        step = -(-length // per_rec)
        rows += [(rec, a, min(a + step, length)) for a in range(0, length, step)]
    return np.array(rows, dtype=np.uint64)


def timed(ctx, names, fn, calls):
    """per timer of `names` the (median, min, max) ms per launch by device events over `calls` calls of fn and the timed launches per
    call; the host-clock ms of the calls"""
    per = {n: [] for n in names}
    counted = {n: set() for n in names}
    host = []
    for _ in range(calls):
        before = {n: ctx.timing(n) for n in names}
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        host.append((time.perf_counter() - t0) * 1e3)
        for n in names:
            ms1, n1 = ctx.timing(n)
            per[n].append((ms1 - before[n][0]) / max(n1 - before[n][1], 1))
            counted[n].add(int(n1 - before[n][1]))
    out = {n: {"median_ms": statistics.median(per[n]), "min_ms": min(per[n]), "max_ms": max(per[n]), "timed_launches_per_call": sorted(counted[n])}
           for n in names}
    out["calls"] = calls
    out["host_ms_median"] = statistics.median(host)
    return out


def measure_hset(ctx, g, bf, iv, tenth, k, calls, out):
    "the set sweep beside the filter sweep: same genome, same intervals, same process"
    rec10, _ = g.bf_sample_intervals(bf, tenth, k, 16)
    members = np.unique(rec10["h0"])
    del rec10
    made = []

    def build():
        made.append(HashSet(ctx, members))
        if len(made) > 1:
            made.pop(0).free()
    out["hset_build"] = dict(timed(ctx, ["hset_build"], build, calls), hashes=int(members.size))
    hset = made[0]
    set_timers, bf_timers = ["hset_sample_count", "hset_sample_write"], ["bf_sample_count", "bf_sample_write"]
    hit, _ = g.hset_sample_intervals(hset, iv, k, 16)           # warm-up, and the record count
    out["hset_sample"] = dict(timed(ctx, set_timers, lambda: g.hset_sample_intervals(hset, iv, k, 16), calls), records=int(hit.size))
    rec, _ = g.bf_sample_intervals(bf, iv, k, 16)
    out["bf_sample"] = dict(timed(ctx, bf_timers, lambda: g.bf_sample_intervals(bf, iv, k, 16), calls), records=int(rec.size))
    both_set = sum(out["hset_sample"][t]["median_ms"] for t in set_timers)
    both_bf = sum(out["bf_sample"][t]["median_ms"] for t in bf_timers)
    out["both_launches_ms"] = {"hset_sample": both_set, "bf_sample": both_bf, "ratio": both_set / both_bf}
    assert all(out["hset_sample"][t]["timed_launches_per_call"] == [1] for t in set_timers), out
    assert all(out["bf_sample"][t]["timed_launches_per_call"] == [1] for t in bf_timers), out
    hset.free()


def counted_sweep(ctx, g, hset, counts, iv, k, calls):
    "hcount_sweep over `iv`, cleared before every call (a 3 Gbp genome offers the counter most of its 2^32); (figures, hits, k-mers)"
    def call():
        counts.clear()
        return g.hset_count_intervals(hset, counts, iv, k, 16)
    hits = int(call().sum())                                    # warm-up, and the hit count
    return dict(timed(ctx, ["hcount_sweep", "hcount_clear"], call, calls), hits=hits), hits


def measure_hcount(ctx, g, bf, iv, tenth, k, calls, out, bp):
    "the counting sweep beside the sampling sweep's count launch: same genome, same set, same tiles, same process"
    rec10, _ = g.bf_sample_intervals(bf, tenth, k, 16)
    members = np.unique(rec10["h0"])
    del rec10
    hset = HashSet(ctx, members)
    counts = HashCounts(ctx, hset)
    out["set_hashes"] = int(members.size)
    set_timers = ["hset_sample_count", "hset_sample_write"]
    g.hset_sample_intervals(hset, iv, k, 16)                    # warm-up
    out["hset_sample"] = timed(ctx, set_timers, lambda: g.hset_sample_intervals(hset, iv, k, 16), calls)
    out["hcount_sweep"], hits = counted_sweep(ctx, g, hset, counts, iv, k, calls)
    top = counts.read(members)
    out["hcount_sweep"].update(largest_count=int(top.max()), members_met=int((top > 0).sum()), counts_sum_equals_hits=bool(int(top.sum()) == hits))
    # the atomics alone: as many member values as the sweep had hits, one add each
    values = np.resize(members, hits)

    def add():
        counts.clear()
        counts.add(values)
    add()
    out["hcount_add"] = dict(timed(ctx, ["hcount_add"], add, calls), values=int(values.size))
    del values
    out["hcount_read"] = dict(timed(ctx, ["hcount_read"], lambda: counts.read(members), calls), values=int(members.size))
    sweep, yard = out["hcount_sweep"]["hcount_sweep"], out["hset_sample"]["hset_sample_count"]
    out["sweep_vs_count_launch"] = {"hcount_sweep_ms": sweep["median_ms"], "hset_sample_count_ms": yard["median_ms"],
                                    "difference_ms": sweep["median_ms"] - yard["median_ms"],
                                    "yardstick_spread_ms": yard["max_ms"] - yard["min_ms"], "hcount_add_ms": out["hcount_add"]["hcount_add"]["median_ms"]}
    assert sweep["timed_launches_per_call"] == [1] and yard["timed_launches_per_call"] == [1], out
    counts.free()
    hset.free()
    g.free()
    bf.free()
    # contention: an assembly-like genome (satellite arrays, repeat families) against the hashes of a tenth of its own sample
    from ntsynt_amd import synth
    plan = synth.realistic_plan(24, bp // 24, 0, SEED)
    ga = Genome.synth_plan(ctx, plan, SEED, 1000, 0.0065, rep=synth.REPEATS, names=plan[2])
    _, nbytes = bf_size_bytes(ga.total_bp, 0.025)
    own = BloomFilter(ctx, nbytes, k)
    own.insert(ga)
    iv_a = np.array([(r, 0, int(n)) for r, n in enumerate(ga.rec_len)], dtype=np.uint64)
    order = np.argsort(-ga.rec_len.astype(np.int64), kind="stable")
    tenth_a, bases = [], 0
    for r in order:                                             # the longest records up to a tenth of the bases
        tenth_a.append(iv_a[r])
        bases += int(ga.rec_len[r])
        if bases >= ga.total_bp // 10:
            break
    rec_a, _ = ga.bf_sample_intervals(own, np.array(tenth_a, dtype=np.uint64), k, 16)
    members_a = np.unique(rec_a["h0"])
    del rec_a
    own.free()
    hset_a = HashSet(ctx, members_a)
    counts_a = HashCounts(ctx, hset_a)
    figures, hits_a = counted_sweep(ctx, ga, hset_a, counts_a, iv_a, k, calls)
    top = counts_a.read(members_a)
    kmers_a = int(ga.valid_kmers(k))
    out["assembly_like"] = dict(figures, bp=int(ga.total_bp), records=int(iv_a.shape[0]), valid_kmers=kmers_a, set_hashes=int(members_a.size),
                                largest_count=int(top.max()), counts_above_1000=int((top > 1000).sum()), adds_to_counts_above_1000=int(top[top > 1000].sum()))
    uni_ns = out["hcount_sweep"]["hcount_sweep"]["median_ms"] * 1e6 / out["kmers"]
    asm_ns = figures["hcount_sweep"]["median_ms"] * 1e6 / kmers_a
    out["contention"] = {"uniform_ns_per_kmer": uni_ns, "assembly_like_ns_per_kmer": asm_ns, "ratio": asm_ns / uni_ns,
                         "uniform_hits_per_kmer": hits / out["kmers"], "assembly_like_hits_per_kmer": hits_a / kmers_a}
    counts_a.free()
    hset_a.free()
    ga.free()


def measure_sites(ctx, g, bf, iv, tenth, k, calls, out, synth, n_intervals, min_hits):
    "the capped sweep beside the set sweep after one count sweep of the same tiles; one nts_iv_sites call beside nts_iv_links on the same lists"
    rec10, _ = g.bf_sample_intervals(bf, tenth, k, 16)
    members = np.unique(rec10["h0"])
    hset = HashSet(ctx, members)
    counts = HashCounts(ctx, hset)
    out["set_hashes"] = int(members.size)
    out["count_hits"] = int(g.hset_count_intervals(hset, counts, iv, k, 16).sum())      # the one count sweep, of the same tiles
    set_timers, cap_timers = ["hset_sample_count", "hset_sample_write"], ["hcount_sample_count", "hcount_sample_write"]
    plain, _ = g.hset_sample_intervals(hset, iv, k, 16)         # warm-up, and the record count
    out["hset_sample"] = dict(timed(ctx, set_timers, lambda: g.hset_sample_intervals(hset, iv, k, 16), calls), records=int(plain.size))
    both = {"hset_sample": sum(out["hset_sample"][t]["median_ms"] for t in set_timers)}
    occurrences = None
    for name, cap in (("cap_16", 16), ("cap_max", (1 << 32) - 1)):
        rec, _ = g.hset_sample_intervals_capped(hset, counts, cap, iv, k, 16)
        out[name] = dict(timed(ctx, cap_timers, lambda cap=cap: g.hset_sample_intervals_capped(hset, counts, cap, iv, k, 16), calls), cap=cap, records=int(rec.size))
        assert all(out[name][t]["timed_launches_per_call"] == [1] for t in cap_timers), out
        both[name] = sum(out[name][t]["median_ms"] for t in cap_timers)
        if cap == 16:
            occurrences = rec
        else:
            assert np.array_equal(rec, plain)                   # the largest cap after a count sweep of the same tiles: the uncapped records
    del plain, rec
    both.update(dependent_count_load_ms=both["cap_max"] - both["hset_sample"], stores_saved_ms=both["cap_max"] - both["cap_16"])
    out["both_launches_ms"] = both
    counts.free()
    hset.free()
    g.free()
    lists = [rec10]
    for j in (1, 2):
        other = synth(j)
        lists.append(other.bf_sample_intervals(bf, tiling(other, n_intervals)[:tenth.shape[0]], k, 16)[0])
        other.free()
    ctx.profile(1)
    links = ctx.iv_links(lists, min_hits)
    out["iv_links"] = dict(timed(ctx, ["iv_links_join", "iv_links_pairs", "iv_links_select"], lambda: ctx.iv_links(lists, min_hits), max(3, calls // 2)),
                           records=[int(x.size) for x in lists], links=int(links.size))
    sites = ctx.iv_sites(lists, occurrences, 1000, min_hits)
    out["iv_sites"] = dict(timed(ctx, ["iv_sites_join", "iv_sites_pairs", "iv_sites_select"], lambda: ctx.iv_sites(lists, occurrences, 1000, min_hits),
                                 max(3, calls // 2)), records=[int(x.size) for x in lists], target_records=int(occurrences.size), sites=int(sites.size),
                           pairs_in_kept_sites=int(sites["hits"].sum()) if sites.size else 0)
    bf.free()


def measure_periods(ctx, g, bf, iv, tenth, k, calls, out):
    "the sampler that probes nothing beside the filter sweep on the same tiles; one nts_iv_periods call on a tenth's records"
    bf_timers, iv_timers = ["bf_sample_count", "bf_sample_write"], ["iv_sample_count", "iv_sample_write"]
    rec, _ = g.bf_sample_intervals(bf, iv, k, 16)               # warm-up, and the record count
    out["bf_sample"] = dict(timed(ctx, bf_timers, lambda: g.bf_sample_intervals(bf, iv, k, 16), calls), records=int(rec.size))
    del rec
    rec, _ = g.sample_intervals(iv, k, 16)
    out["iv_sample"] = dict(timed(ctx, iv_timers, lambda: g.sample_intervals(iv, k, 16), calls), records=int(rec.size))
    del rec
    assert all(out["bf_sample"][t]["timed_launches_per_call"] == [1] for t in bf_timers), out
    assert all(out["iv_sample"][t]["timed_launches_per_call"] == [1] for t in iv_timers), out
    out["launch_by_launch"] = {}
    for mine, theirs in zip(iv_timers, bf_timers):
        a, b = out["iv_sample"][mine], out["bf_sample"][theirs]
        out["launch_by_launch"][mine] = {"median_ms": a["median_ms"], "yardstick_median_ms": b["median_ms"], "difference_ms": a["median_ms"] - b["median_ms"],
                                         "spread_ms": max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])}
    rec10, _ = g.sample_intervals(tenth, k, 16)
    n_iv = int(tenth.shape[0])
    ctx.profile(1)
    found = ctx.iv_periods(rec10, n_iv)
    out["iv_periods"] = dict(timed(ctx, ["iv_periods_sort", "iv_periods_mode", "iv_periods_extent"], lambda: ctx.iv_periods(rec10, n_iv), calls),
                             records=int(rec10.size), intervals=n_iv, recurring=int(found["recurring"].sum()),
                             intervals_with_4_hits=int((found["period_hits"] >= 4).sum()))


def measure_families(ctx, g, iv, tenth, k, calls, out):
    "the three calls of the gap families on a tenth's unfiltered records, beside nts_iv_periods and nts_iv_sites on lists of the same size"
    rec10, _ = g.sample_intervals(tenth, k, 16)
    n_iv = int(tenth.shape[0])
    ctx.profile(1)
    found = ctx.iv_periods(rec10, n_iv)
    out["iv_periods"] = dict(timed(ctx, ["iv_periods_sort", "iv_periods_mode", "iv_periods_extent"], lambda: ctx.iv_periods(rec10, n_iv), calls),
                             records=int(rec10.size), intervals=n_iv)
    period = np.where(found["period_hits"] >= 4, found["period"], 0).astype(np.uint32)
    carried = ctx.iv_period_hashes(rec10, n_iv, period)
    out["iv_period_hashes"] = dict(timed(ctx, ["iv_phash"], lambda: ctx.iv_period_hashes(rec10, n_iv, period), calls), records=int(rec10.size),
                                   intervals_with_a_period=int((period > 0).sum()), lines=int(carried.size))
    family, hashes, hash_family = ctx.iv_families(rec10, n_iv)  # (every record a pair: the join on a list of the yardstick's size)
    out["iv_families"] = dict(timed(ctx, ["iv_families_join"], lambda: ctx.iv_families(rec10, n_iv), calls), pairs=int(rec10.size), arrays=n_iv,
                              families=int(np.unique(family).size), hashes=int(hashes.size))
    hset = HashSet(ctx, hashes)
    occurrences, _ = g.hset_sample_intervals(hset, iv, k, 16)   # the whole genome against the set
    hset.free()
    sites = ctx.iv_family_sites(occurrences, hashes, hash_family, 1000, 4)
    out["iv_family_sites"] = dict(timed(ctx, ["iv_family_sites_label", "iv_family_sites_select"],
                                        lambda: ctx.iv_family_sites(occurrences, hashes, hash_family, 1000, 4), calls), occurrences=int(occurrences.size),
                                  hashes=int(hashes.size), sites=int(sites.size))
    found_sites = ctx.iv_sites([rec10], occurrences, 1000, 4)
    out["iv_sites"] = dict(timed(ctx, ["iv_sites_join", "iv_sites_pairs", "iv_sites_select"], lambda: ctx.iv_sites([rec10], occurrences, 1000, 4), calls),
                           records=int(rec10.size), target_records=int(occurrences.size), sites=int(found_sites.size))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--bp", type=int, default=3_000_000_000)
    p.add_argument("--k", type=int, default=24)
    p.add_argument("--calls", type=int, default=6)
    p.add_argument("--intervals", type=int, default=10_000)
    p.add_argument("--min-anchors", type=int, default=4)
    p.add_argument("--no-join", action="store_true", help="the sampling launches only")
    p.add_argument("--hset", action="store_true", help="the set sweep of gap block links beside the filter sweep, and nothing else")
    p.add_argument("--hcount", action="store_true", help="the counting sweep of gap copies beside the set sweep's count launch, and nothing else")
    p.add_argument("--sites", action="store_true", help="the capped sweep of gap copy sites beside the set sweep, the site join beside the link join, and nothing else")
    p.add_argument("--periods", action="store_true", help="the sampler without a filter of gap periods beside the filter sweep, one nts_iv_periods call, and nothing else")
    p.add_argument("--families", action="store_true", help="the three calls of gap families beside nts_iv_periods and nts_iv_sites on lists of the same size, and nothing else")
    p.add_argument("--out")
    args = p.parse_args()
    k = args.k
    ctx = Context(0)
    synth = lambda j: Genome.synth(ctx, args.bp, 24, SEED, 1000 + j, DIVERGENCE)      # noqa: E731
    g = synth(0)
    _, nbytes = bf_size_bytes(g.total_bp, 0.025)
    bf = BloomFilter(ctx, nbytes, k)
    bf.insert(g)
    for j in (1, 2):                                            # the family's other two genomes, one resident at a time
        other = synth(j)
        bf.insert_and(other)
        other.free()
    out = {"bp": args.bp, "k": k, "filter_bytes": nbytes, "occupancy": bf.get_fpr(), "valid_kmers": g.valid_kmers(k)}
    iv = tiling(g, args.intervals)
    tenth = iv[:max(1, iv.shape[0] // 10)]
    ctx.profile(2)
    kmers, hits = g.bf_count_intervals(bf, iv, k)             # warm-up, and the figures themselves
    out["intervals"], out["kmers"], out["held"] = int(iv.shape[0]), int(kmers.sum()), int(hits.sum())
    if args.families:
        measure_families(ctx, g, iv, tenth, k, args.calls, out)
        ctx.profile(False)
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w", encoding="utf-8") as fh:
                fh.write(text + "\n")
        g.free()
        bf.free()
        ctx.close()
        return
    if args.periods:
        measure_periods(ctx, g, bf, iv, tenth, k, args.calls, out)
        ctx.profile(False)
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w", encoding="utf-8") as fh:
                fh.write(text + "\n")
        g.free()
        bf.free()
        ctx.close()
        return
    if args.sites:
        measure_sites(ctx, g, bf, iv, tenth, k, args.calls, out, synth, args.intervals, args.min_anchors)     # (frees the genome and the filter)
        ctx.profile(False)
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w", encoding="utf-8") as fh:
                fh.write(text + "\n")
        ctx.close()
        return
    if args.hcount:
        measure_hcount(ctx, g, bf, iv, tenth, k, args.calls, out, args.bp)     # (frees the genome and the filter: it loads another pair)
        ctx.profile(False)
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w", encoding="utf-8") as fh:
                fh.write(text + "\n")
        ctx.close()
        return
    if args.hset:
        measure_hset(ctx, g, bf, iv, tenth, k, args.calls, out)
        ctx.profile(False)
        text = json.dumps(out, indent=1)
        print(text)
        if args.out:
            with open(args.out, "w", encoding="utf-8") as fh:
                fh.write(text + "\n")
        g.free()
        bf.free()
        ctx.close()
        return
    # the yardstick: the counting launch, which probes every k-mer
    out["bf_count_iv"] = timed(ctx, ["bf_count_iv"], lambda: g.bf_count_intervals(bf, iv, k), args.calls)
    sample_timers = ["bf_sample_count", "bf_sample_write"]
    rec, _ = g.bf_sample_intervals(bf, iv, k, 16)
    out["rate16"] = dict(timed(ctx, sample_timers, lambda: g.bf_sample_intervals(bf, iv, k, 16), args.calls), records=int(rec.size))
    both = out["rate16"]["bf_sample_count"]["median_ms"] + out["rate16"]["bf_sample_write"]["median_ms"]
    out["rate16"]["both_launches_ms"] = both
    out["rate16"]["ratio_to_count_launch"] = both / out["bf_count_iv"]["bf_count_iv"]["median_ms"]
    k10, h10 = g.bf_count_intervals(bf, tenth, k)
    out["tenth"] = {"intervals": int(tenth.shape[0]), "kmers": int(k10.sum()), "held": int(h10.sum()),
                    "bf_count_iv": timed(ctx, ["bf_count_iv"], lambda: g.bf_count_intervals(bf, tenth, k), args.calls)}
    r1, _ = g.bf_sample_intervals(bf, tenth, k, 1)
    assert r1.size == int(h10.sum())
    out["tenth"]["rate1"] = dict(timed(ctx, sample_timers, lambda: g.bf_sample_intervals(bf, tenth, k, 1), args.calls), records=int(r1.size))
    del r1
    out["tenth"]["rate16"] = timed(ctx, sample_timers, lambda: g.bf_sample_intervals(bf, tenth, k, 16), args.calls)
    if not args.no_join:
        # three such lists: every genome of the family sampled over its own tiling, joined
        lists = [rec]
        g.free()
        for j in (1, 2):
            other = synth(j)
            lists.append(other.bf_sample_intervals(bf, tiling(other, args.intervals), k, 16)[0])
            other.free()
        join_timers = ["iv_links_join", "iv_links_pairs", "iv_links_select"]
        ctx.profile(1)
        links = ctx.iv_links(lists, args.min_anchors)
        out["join"] = dict(timed(ctx, join_timers, lambda: ctx.iv_links(lists, args.min_anchors), max(3, args.calls // 2)),
                           records=[int(x.size) for x in lists], links=int(links.size), anchors=int(links["anchors"].sum()) if links.size else 0)
    else:
        g.free()
    ctx.profile(False)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as fh:
            fh.write(text + "\n")
    # the comparison holds only if each call timed exactly one launch of each kernel
    assert out["bf_count_iv"]["bf_count_iv"]["timed_launches_per_call"] == [1], out
    assert all(out["rate16"][t]["timed_launches_per_call"] == [1] for t in sample_timers), out
    bf.free()
    ctx.close()


if __name__ == "__main__":
    main()

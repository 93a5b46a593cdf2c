"""The gap periods by their definitions (docs/design/04_14_gap_periods.md), over dictionaries: what tests/test_gpu_iv_periods.py and
tests/test_gpu_gap_periods.py compare the device's answers and the written file with.  No GPU, no library of the project."""
import numpy as np

U64_MAX = (1 << 64) - 1
FIELDS = ("recurring", "period", "period_hits", "first_off", "last_off")


def brute_periods(records, n_iv):
    """records: (h0, iv, off) triples in any order; returns one (recurring, period, period_hits, first_off, last_off) per interval.
    Per interval and hash the offsets in ascending order; every one but the first has the lag to its predecessor; the period is the
    lag held by the most records, the smallest on a tie; the extent runs from the smallest off - period to the largest off over the
    records whose lag is the period.  All zeros where nothing recurs."""
    offs = [dict() for _ in range(n_iv)]                        # interval -> hash -> [off]
    for h0, iv, off in records:
        offs[int(iv)].setdefault(int(h0), []).append(int(off))
    out = []
    for by_hash in offs:
        lagged = []                                             # (lag, off) of every record that has a lag
        for lst in by_hash.values():
            lst.sort()
            lagged += [(b - a, b) for a, b in zip(lst, lst[1:])]
        if not lagged:
            out.append((0, 0, 0, 0, 0))
            continue
        held = {}
        for lag, _ in lagged:
            held[lag] = held.get(lag, 0) + 1
        hits, period = max((n, -lag) for lag, n in held.items())
        period = -period
        at = [off for lag, off in lagged if lag == period]
        out.append((len(lagged), period, hits, min(at) - period, max(at)))
    return out


def ratio(x):
    "the ratios of the gap files: six significant digits"
    return f"{x:.6g}"


def brute_line(gap, k, sampled, result, min_hits):
    "the nine columns behind the first six of a gap's line: gap = (genome, contig, start, end, kind)"
    _, _, start, end, _ = gap
    recurring, period, hits, first_off, last_off = result
    if hits < min_hits:
        return [str(sampled), str(recurring), ".", str(hits), ".", ".", ".", ".", "."]
    lo, hi = start + first_off, start + last_off + k
    covered, length = hi - lo, end - start
    tenths = (10 * covered) // period
    return [str(sampled), str(recurring), str(period), str(hits), str(lo), str(hi), f"{tenths // 10}.{tenths % 10}", ratio(covered / length),
            "tandem" if 2 * covered > length else "partial"]


def brute_file(gaps, kmers_of, k, rate, min_hits):
    """the text of <prefix>.gap_periods.tsv: gaps = (genome, contig, start, end, kind) in the file's order; kmers_of(genome, contig) =
    (positions, canonical hashes) of every valid k-mer of that record.  Returns (text, {gap: (sampled, result)})."""
    thresh = U64_MAX // rate
    lines = ["\t".join(("genome", "contig", "start", "end", "length", "kind", "sampled", "recurring", "period", "period_hits", "from", "to", "copies",
                        "covered_fraction", "class"))]
    facts = {}
    for gap in gaps:
        genome, contig, start, end, kind = gap
        pos, h0 = kmers_of(genome, contig)
        records = [(int(h), 0, int(p) - start) for p, h in zip(pos, h0) if p >= start and p + k <= end and int(h) <= thresh]
        result = brute_periods(records, 1)[0]
        facts[gap] = (len(records), result)
        lines.append("\t".join([genome, contig, str(start), str(end), str(end - start), kind] + brute_line(gap, k, len(records), result, min_hits)))
    lines.append(f"# k {k}, rate {rate}, min_hits {min_hits}")
    return "\n".join(lines) + "\n", facts


def as_array(results):
    "brute_periods' tuples as the device's record array"
    out = np.zeros(len(results), dtype=np.dtype([(n, "<u4") for n in FIELDS]))
    for i, r in enumerate(results):
        out[i] = r
    return out

"""The gap families by their definitions (docs/design/04_15_gap_families.md), over dictionaries and a plain union-find: what
tests/test_gpu_iv_period_hashes.py, tests/test_gpu_iv_families.py, tests/test_gpu_iv_family_sites.py and tests/test_gpu_gap_families.py
compare the device's answers and the two written files with.  No GPU, no library of the project."""
import numpy as np

from tests.periods_brute import brute_periods

U64_MAX = (1 << 64) - 1
SAMPLE = np.dtype([("h0", "<u8"), ("iv", "<u4"), ("off", "<u4")])
FSITE = np.dtype([(n, "<u4") for n in ("family", "rec", "first", "last", "hits")])
FAMILY_HEADER = ("genome", "contig", "start", "end", "length", "kind", "period", "class", "family", "members", "genomes", "array_hashes", "shared_hashes")
SITE_HEADER = ("family", "genome", "contig", "from", "to", "length", "hits", "period", "period_hits", "copies", "blocks", "placement")


def brute_period_hashes(records, n_iv, period):
    """records: (h0, iv, off) triples in any order; period: one per interval, 0 = skip.  Returns the sorted list of (iv, h0, count):
    per interval and hash the offsets ascending, every one but the first has the lag to its predecessor; count = the records whose lag
    is the interval's period; only counts above zero"""
    offs = {}
    for h0, iv, off in records:
        offs.setdefault((int(iv), int(h0)), []).append(int(off))
    out = []
    for (iv, h0), lst in offs.items():
        assert iv < n_iv
        lst.sort()
        count = sum(1 for a, b in zip(lst, lst[1:]) if period[iv] and b - a == period[iv])
        if count:
            out.append((iv, h0, count))
    return sorted(out)


def brute_families(pairs, n_arrays):
    """pairs: (h0, array) in any order, duplicates allowed.  Returns (family, hashes, hash_family): family[a] = the smallest array of
    a's connected component under "two arrays have a hash in common", the distinct hashes ascending, the component of each"""
    parent = list(range(n_arrays))

    def root(a):
        while parent[a] != a:
            a = parent[a]
        return a
    holder = {}
    for h0, a in pairs:
        h0, a = int(h0), int(a)
        if h0 in holder:
            x, y = root(holder[h0]), root(a)
            parent[max(x, y)] = min(x, y)
        else:
            holder[h0] = a
    family = [root(a) for a in range(n_arrays)]
    hashes = sorted(holder)
    return family, hashes, [family[holder[h]] for h in hashes]


def brute_family_sites(occurrences, family_of, step, min_hits):
    """occurrences: (h0, rec, pos) triples in any order; family_of: {h0: family}.  Returns the sorted list of (family, rec, first, last,
    hits): within one family the occurrences by (rec, pos); a site is a maximal run within one record whose consecutive positions
    differ by at most step; kept with at least min_hits occurrences"""
    by_family = {}
    for h0, rec, pos in occurrences:
        if int(h0) in family_of:
            by_family.setdefault(family_of[int(h0)], []).append((int(rec), int(pos)))
    out = []
    for fam, lst in by_family.items():
        lst.sort()
        run = [lst[0]]
        for cur in lst[1:] + [None]:
            if cur is not None and cur[0] == run[-1][0] and cur[1] - run[-1][1] <= step:
                run.append(cur)
                continue
            if len(run) >= min_hits:
                out.append((fam, run[0][0], run[0][1], run[-1][1], len(run)))
            run = [cur]
    return sorted(out)


def as_samples(triples):
    "(iv, h0, off) triples as the device's record array"
    out = np.zeros(len(triples), dtype=SAMPLE)
    for i, (iv, h0, off) in enumerate(triples):
        out[i] = (h0, iv, off)
    return out


def as_sites(rows):
    out = np.zeros(len(rows), dtype=FSITE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def brute_files(gaps, period_lines, kmers_of, records_of, blocks, k, rate, min_hits, step):
    """the texts of <prefix>.gap_families.tsv and <prefix>.gap_family_sites.tsv.  gaps = (genome, contig, start, end, kind) in the
    order of gap_periods.tsv; period_lines = that file's lines split into fields, one per gap; kmers_of(genome, contig) = (positions,
    canonical hashes) of every valid k-mer of that record; records_of = {genome: [contig, ...] in file order}; blocks = rows with
    genome, contig, start, end, block_id in the block table's order.  Returns (families text, sites text, facts) with facts =
    {"family_of_array": [...], "arrays": [gap, ...], "sites": [(family, genome, contig, from, to, hits, placement), ...]}."""
    thresh = U64_MAX // rate
    arrays = [i for i, f in enumerate(period_lines) if f[14] in ("tandem", "partial")]
    pairs, hashes_of = [], []
    for a, i in enumerate(arrays):
        genome, contig, start, end, _ = gaps[i]
        pos, h0 = kmers_of(genome, contig)
        recs = [(int(h), 0, int(p) - start) for p, h in zip(pos, h0) if p >= start and p + k <= end and int(h) <= thresh]
        mine = {h for _, h, _ in brute_period_hashes(recs, 1, [int(period_lines[i][8])])}
        hashes_of.append(mine)
        pairs += [(h, a) for h in sorted(mine)]
    family, hashes, hash_family = brute_families(pairs, len(arrays))
    number = {root: n + 1 for n, root in enumerate(sorted(set(family)))}
    lines = ["\t".join(FAMILY_HEADER)]
    for a, i in enumerate(arrays):
        members = [b for b in range(len(arrays)) if family[b] == family[a]]
        shared = sum(1 for h in hashes_of[a] if any(h in hashes_of[b] for b in range(len(arrays)) if b != a))
        f = period_lines[i]
        lines.append("\t".join(f[:6] + [f[8], f[14], str(number[family[a]]), str(len(members)), str(len({gaps[arrays[b]][0] for b in members})),
                                        str(len(hashes_of[a])), str(shared)]))
    footer = f"# k {k}, rate {rate}, min_hits {min_hits}, step {step}, arrays {len(arrays)}, families {len(number)}, set {len(hashes)} hashes"
    lines.append(footer)
    family_of = {h: number[f] for h, f in zip(hashes, hash_family)}
    site_lines, sites = ["\t".join(SITE_HEADER)], []
    keyed = []
    for genome in sorted(records_of):
        occ = []
        for rec, contig in enumerate(records_of[genome]):
            pos, h0 = kmers_of(genome, contig)
            occ += [(int(h), rec, int(p)) for p, h in zip(pos, h0) if int(h) <= thresh and int(h) in family_of]
        for fam, rec, first, last, hits in brute_family_sites(occ, family_of, step, min_hits):
            inside = [(h, 0, p - first) for h, r, p in occ if family_of[h] == fam and r == rec and first <= p <= last]
            _, period, period_hits, _, _ = brute_periods(inside, 1)[0]
            keyed.append(((fam, genome, rec, first), (last, hits, period, period_hits)))
    for (fam, genome, rec, first), (last, hits, period, period_hits) in sorted(keyed):
        contig, to = records_of[genome][rec], last + k
        if period_hits < min_hits:
            per = [".", ".", "."]
        else:
            tenths = (10 * (to - first)) // period
            per = [str(period), str(period_hits), f"{tenths // 10}.{tenths % 10}"]
        ids = []
        for b in blocks:
            if b.genome == genome and b.contig == contig and b.start < to and b.end > first and b.block_id not in ids:
                ids.append(b.block_id)

        def touched(which):
            return any(g[0] == genome and g[1] == contig and first < g[3] and to > g[2] for g in which)
        member_gaps = [gaps[arrays[a]] for a in range(len(arrays)) if number[family[a]] == fam]
        place = "array" if touched(member_gaps) else "gap" if touched(gaps) else "block"
        site_lines.append("\t".join([str(fam), genome, contig, str(first), str(to), str(to - first), str(hits)] + per + [",".join(ids) or ".", place]))
        sites.append((fam, genome, contig, first, to, hits, place))
    site_lines.append(footer)
    facts = {"family_of_array": [number[f] for f in family], "arrays": [gaps[i] for i in arrays], "sites": sites}
    return "\n".join(lines) + "\n", "\n".join(site_lines) + "\n", facts

"""What a run's synteny blocks leave out, and how much of it every genome shares (`ntSynt --gaps`, bin/ntsynt_gaps).

Per genome and record the complement of the blocks' intervals is cut into gaps (cut: host arithmetic; no GPU, no torch, no numpy), and
for every gap -- and, as the baseline, for every merged in-block interval -- the k-mers that the run's common Bloom filter holds are
counted on the GPU in one sweep per genome (report: nts_bf_count_intervals).  A gap whose k-mers are mostly in the filter is sequence
every genome has and the chaining dropped; one at the filter's occupancy is the genome's own; one without valid k-mers is an assembly
gap.  docs/design/04_9_gap_content.md.

Where a gap's shared sequence lies in the other genomes (`ntSynt --gap-links`, `bin/ntsynt_gaps --links-out`): a thin sample of the gap
k-mers the filter holds is taken per genome (links: nts_bf_sample_intervals over the gaps only) and joined across genomes by hash on
the GPU (nts_iv_links); a pair of gaps of two genomes with enough hashes in common is a link, with its orientation from the order of
the anchors and its placement from the gaps' flanking blocks.  docs/design/04_10_gap_links.md.

Where it lies INSIDE the blocks, the gap's own genome included (`ntSynt --gap-block-links`, `bin/ntsynt_gaps --block-links-out`): the
gaps' sampled hashes become an exact hash set on the GPU (nts_hset_build), every genome's merged block intervals are swept against it
(block_links: nts_hset_sample_intervals writes only the hits) and the same join links gaps to block intervals.
docs/design/04_11_gap_block_links.md.

How often each genome holds a gap's sampled k-mers, genome-wide (`ntSynt --gap-copies`, `bin/ntsynt_gaps --copies-out`): the same set
gets a table of counts beside it (nts_hcount_create), every genome is swept WHOLE against it (copies: nts_hset_count_intervals adds 1
per occurrence) and the counts are read back by hash; a gap whose sampled k-mers occur once in every genome could have been chained, one
whose k-mers its own genome holds several times is a repeat and no threshold brings it back (copy_stats).
docs/design/04_12_gap_copies.md.

WHERE each genome holds those copies (`ntSynt --gap-copy-sites`, `bin/ntsynt_gaps --copy-sites-out`): behind a genome's count sweep the
same genome is swept once more and the positions of the members whose count lies in 1..cap are written
(nts_hset_sample_intervals_capped), then joined against the gaps' records with multiplicity allowed on both sides and grouped into
sites (copy_sites: nts_iv_sites, one call per target genome).  docs/design/04_13_gap_copy_sites.md.

Which gaps are tandem arrays (`ntSynt --gap-periods`, `bin/ntsynt_gaps --periods-out`): every genome's gaps are sampled once more
WITHOUT any filter (sample_all: nts_sample_intervals -- an array that one genome alone has is in no common filter), and per genome one
call finds, for every gap, the distance that most often separates two consecutive copies of a sampled k-mer (periods: nts_iv_periods):
the period, how many records hold it, and the stretch they cover.  docs/design/04_14_gap_periods.md.

Which of those arrays are the same satellite, and where else a genome holds it (`ntSynt --gap-families`, `bin/ntsynt_gaps
--families-out / --family-sites-out`): every array is reduced to the distinct hashes that carry its period (nts_iv_period_hashes), the
arrays that share a hash are joined into families (nts_iv_families), the hashes become an exact set, every genome is swept WHOLE against
it (nts_hset_sample_intervals) and its occurrences fall into sites per family (families: nts_iv_family_sites, then nts_iv_periods on
the kept sites) -- a join that is linear in the occurrences.  docs/design/04_15_gap_families.md."""
import os
from collections import namedtuple

GAP_COLUMNS = ("genome", "contig", "start", "end", "length", "kind", "left_block", "right_block", "n_bases", "kmers", "shared_kmers",
               "shared_fraction", "excess")
SUMMARY_COLUMNS = ("genome", "part", "intervals", "bases", "n_bases", "kmers", "shared_kmers", "shared_fraction", "excess")

LINK_COLUMNS = ("genome_a", "contig_a", "start_a", "end_a", "left_a", "right_a", "genome_b", "contig_b", "start_b", "end_b", "left_b", "right_b",
                "anchors", "orientation", "from_a", "to_a", "from_b", "to_b", "sampled_a", "sampled_b", "placement")
LINKS_RATE, LINKS_MIN = 16, 4                                   # --gap-links-rate / --gap-links-min
BLOCK_LINK_COLUMNS = ("genome", "contig", "start", "end", "left_block", "right_block", "target_genome", "target_contig", "target_start", "target_end",
                      "blocks", "anchors", "orientation", "from", "to", "from_t", "to_t", "sampled", "target_hits", "placement")
COPY_COLUMNS = ("genome", "contig", "start", "end", "left_block", "right_block", "sampled", "single_own", "single_all", "absent_some",
                "copies_own_median", "copies_own_max", "copies_any_median", "class")
SITE_COLUMNS = ("genome", "contig", "start", "end", "left_block", "right_block", "class", "target_genome", "target_contig", "from_t", "to_t", "blocks",
                "hits", "orientation", "from", "to", "sampled", "usable", "placement")
PERIOD_COLUMNS = ("genome", "contig", "start", "end", "length", "kind", "sampled", "recurring", "period", "period_hits", "from", "to", "copies",
                  "covered_fraction", "class")
FAMILY_COLUMNS = ("genome", "contig", "start", "end", "length", "kind", "period", "class", "family", "members", "genomes", "array_hashes",
                  "shared_hashes")
FAMILY_SITE_COLUMNS = ("family", "genome", "contig", "from", "to", "length", "hits", "period", "period_hits", "copies", "blocks", "placement")
SITES_CAP, SITES_STEP = 16, 1000                                # --gap-sites-cap / --gap-sites-step
MAX_BLOCK_LINK_GENOMES = 32                                     # nts_iv_links takes at most 64 lists: every genome's gaps and its blocks

# a stretch of `contig` of `genome` outside every block: [start, end); kind: between / leading / trailing / unplaced (the record has no
# block at all); left_block / right_block: the block that ends at `start` / starts at `end`, "." where there is none
Gap = namedtuple("Gap", ["genome", "contig", "start", "end", "kind", "left_block", "right_block"])
# the union of the blocks' intervals, overlapping and touching ones merged
Merged = namedtuple("Merged", ["genome", "contig", "start", "end"])


def read_fai(path):
    "[(record name, length)] of a .fai file, in file order"
    out = []
    with open(path, "r", encoding="utf-8") as fh:
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if len(f) >= 2:
                out.append((f[0], int(f[1])))
    return out


def cut(blocks, records):
    """blocks: assess.read_blocks' rows; records: {genome name: [(record name, length), ...] in file order}.  Returns (gaps, merged):
    per genome and record the union of the blocks' intervals clipped to the record (merged) and its complement (gaps; none of length
    zero).  Genomes by name ascending, records in file order, gaps by start.  A genome of `records` the table does not name has
    every record unplaced; a block on a genome or record that `records` does not have is an error.  On ties the first block in file
    order names left_block / right_block."""
    placed = {}                                                 # genome -> contig -> [(start, end, file index, block id)]
    for i, r in enumerate(blocks):
        if r.genome not in records:
            raise ValueError(f"block table names genome {r.genome}, which is not among {sorted(records)}")
        placed.setdefault(r.genome, {}).setdefault(r.contig, []).append((r.start, r.end, i, r.block_id))
    gaps, merged = [], []
    for genome in sorted(records):
        lengths = dict(records[genome])
        for contig in placed.get(genome, {}):
            if contig not in lengths:
                raise ValueError(f"block table names record {contig} of genome {genome}, which that genome does not have")
        for contig, length in records[genome]:
            rows = []
            for start, end, i, bid in placed.get(genome, {}).get(contig, []):
                start, end = max(start, 0), min(end, length)
                if end > start:
                    rows.append((start, end, i, bid))
            if not rows:
                if length > 0:
                    gaps.append(Gap(genome, contig, 0, length, "unplaced", ".", "."))
                continue
            rows.sort(key=lambda t: (t[0], t[2]))
            runs = []                                           # [start, end, id of the first block that starts at start, .. ends at end]
            for start, end, i, bid in rows:
                if runs and start <= runs[-1][1]:
                    run = runs[-1]
                    if end > run[1] or (end == run[1] and i < run[4]):
                        run[1], run[3], run[4] = end, bid, i
                else:
                    runs.append([start, end, bid, bid, i])
            at, left = 0, "."
            for n, (start, end, first_id, last_id, _) in enumerate(runs):
                if start > at:
                    gaps.append(Gap(genome, contig, at, start, "between" if n else "leading", left, first_id))
                merged.append(Merged(genome, contig, start, end))
                at, left = end, last_id
            if length > at:
                gaps.append(Gap(genome, contig, at, length, "trailing", left, "."))
    return gaps, merged


def excess(shared, kmers, occupancy):
    """the share of the k-mers the filter holds beyond what its false positives alone give: max(0, (shared / kmers - occ) / (1 - occ));
    None without k-mers; 0 for a full filter (occ = 1: every answer is a false positive)"""
    if kmers == 0:
        return None
    if occupancy >= 1.0:
        return 0.0
    return max(0.0, (shared / kmers - occupancy) / (1.0 - occupancy))


def _ratio(x):
    return "NA" if x is None else f"{x:.6g}"


def _footer(k, bits, occupancy):
    return f"# k {int(k)}, filter {int(bits)} bits, occupancy {occupancy:.6g}"


def table(rows, k, bits, occupancy):
    "<prefix>.gaps.tsv: a header, one line per gap (report()'s gap rows), then `# k K, filter BITS bits, occupancy OCC`"
    lines = ["\t".join(GAP_COLUMNS)]
    for r in rows:
        frac = None if r["kmers"] == 0 else r["shared_kmers"] / r["kmers"]
        lines.append("\t".join([r["genome"], r["contig"], str(r["start"]), str(r["end"]), str(r["end"] - r["start"]), r["kind"], r["left_block"],
                                r["right_block"], str(r["n_bases"]), str(r["kmers"]), str(r["shared_kmers"]), _ratio(frac),
                                _ratio(excess(r["shared_kmers"], r["kmers"], occupancy))]))
    lines.append(_footer(k, bits, occupancy))
    return "\n".join(lines) + "\n"


def summary(gap_rows, block_rows, k, bits, occupancy, genomes=None):
    """<prefix>.gap_summary.tsv: per genome (ascending; `genomes` names those without a row of either kind) a line `in_blocks` over the
    merged in-block intervals and a line `outside` over the gaps, then the footer of table().  A k-mer that straddles a block's end
    lies wholly inside neither an interval nor a gap and is counted in neither line."""
    names = sorted(set(genomes or ()) | {r["genome"] for r in gap_rows} | {r["genome"] for r in block_rows})
    lines = ["\t".join(SUMMARY_COLUMNS)]
    for name in names:
        for part, rows in (("in_blocks", block_rows), ("outside", gap_rows)):
            mine = [r for r in rows if r["genome"] == name]
            kmers, shared = sum(r["kmers"] for r in mine), sum(r["shared_kmers"] for r in mine)
            frac = None if kmers == 0 else shared / kmers
            lines.append("\t".join([name, part, str(len(mine)), str(sum(r["end"] - r["start"] for r in mine)), str(sum(r["n_bases"] for r in mine)),
                                    str(kmers), str(shared), _ratio(frac), _ratio(excess(shared, kmers, occupancy))]))
    lines.append(_footer(k, bits, occupancy))
    return "\n".join(lines) + "\n"


def report(ctx, genomes_by_name, bf, k, blocks):
    """(gap rows, in-block rows, filter bits, occupancy): cut()'s gaps and merged intervals as dicts with n_bases, kmers and
    shared_kmers added.  genomes_by_name: the name in column 2 of the table -> resident device.Genome, or a callable that returns
    one (it is then freed after its sweep: one genome resident at a time).  bf: the common filter (device.BloomFilter), built with
    this k.  One nts_bf_count_intervals call per genome, its gaps and its merged block intervals together.  ctx is not used: every
    call goes through the context the genome and the filter were made on (the argument mirrors assess.block_divergence)."""
    for r in blocks:
        if r.genome not in genomes_by_name:
            raise ValueError(f"block table names genome {r.genome}, which is not among {sorted(genomes_by_name)}")
    bits = int(bf.bytes) * 8
    occupancy = bf.popcount() / float(bits)
    gap_rows, block_rows = [], []
    for name in sorted(genomes_by_name):
        g = genomes_by_name[name]
        loaded = callable(g)
        if loaded:
            g = g()
        try:
            rec_of = {c: j for j, c in enumerate(g.names)}
            gaps, merged = cut([r for r in blocks if r.genome == name], {name: [(c, int(n)) for c, n in zip(g.names, g.rec_len)]})
            both = gaps + merged
            iv = [(rec_of[r.contig], r.start, r.end) for r in both]
            kmers, hits = g.bf_count_intervals(bf, iv, k)
            valid = g.valid_bases(iv)
        finally:
            if loaded:
                g.free()
        for q, r in enumerate(both):
            row = dict(r._asdict(), n_bases=(r.end - r.start) - int(valid[q]), kmers=int(kmers[q]), shared_kmers=int(hits[q]))
            (gap_rows if q < len(gaps) else block_rows).append(row)
    return gap_rows, block_rows, bits, occupancy


def report_texts(ctx, genomes_by_name, bf, k, blocks):
    "(text of <prefix>.gaps.tsv, text of <prefix>.gap_summary.tsv)"
    gap_rows, block_rows, bits, occupancy = report(ctx, genomes_by_name, bf, k, blocks)
    return table(gap_rows, k, bits, occupancy), summary(gap_rows, block_rows, k, bits, occupancy, genomes=list(genomes_by_name))


def orientation(fwd, rev):
    """of a link, from its anchors ordered by their offset in gap a: `+` when more consecutive pairs rise in gap b than fall, `-` when
    more fall, `.` otherwise (a single anchor included).  The canonical hash carries no strand; the order of the anchors does."""
    return "+" if fwd > rev else "-" if rev > fwd else "."


def placement(a, b):
    """`same` when the two gaps (rows with left_block / right_block) lie between the same two blocks, in either order -- an inversion
    or an eroded block --, `other` otherwise -- a translocation; a pair of gaps without any flanking block is never `same`"""
    fa, fb = {a["left_block"], a["right_block"]}, {b["left_block"], b["right_block"]}
    return "same" if fa == fb and fa != {"."} else "other"


def _each_genome(genomes_by_name, names, sweep):
    "sweep(name, resident genome) per genome in the order of `names`; one given as a loader is loaded for its sweep and freed after it"
    for name in names:
        g = genomes_by_name[name]
        loaded = callable(g)
        if loaded:
            g = g()
        try:
            sweep(name, g)
        finally:
            if loaded:
                g.free()


def _interval_rows(g, rows):
    rec_of = {c: j for j, c in enumerate(g.names)}
    return [(rec_of[r["contig"]], r["start"], r["end"]) for r in rows]


def sample_gaps(genomes_by_name, bf, k, gap_rows, rate=LINKS_RATE):
    """(lists, sampled): per genome, ascending by name, the records and the per-gap counts of one nts_bf_sample_intervals call over
    its gaps only (the k-mers the filter holds with h0 <= (2^64 - 1) // rate).  gap_rows are report()'s (every genome's, in its
    order); genomes_by_name and bf as for report().  One sampling serves links() and block_links()."""
    if rate < 1:
        raise ValueError("sample_gaps: rate must be at least 1")
    lists, sampled = [], []

    def sweep(name, g):
        rec, counts = g.bf_sample_intervals(bf, _interval_rows(g, [r for r in gap_rows if r["genome"] == name]), k, rate)
        lists.append(rec)
        sampled.append(counts)
    _each_genome(genomes_by_name, sorted(genomes_by_name), sweep)
    return lists, sampled


def links(ctx, genomes_by_name, bf, k, gap_rows, rate=LINKS_RATE, min_anchors=LINKS_MIN, sampling=None):
    """the links between the gaps of different genomes: gap_rows are report()'s (every genome's, in its order); genomes_by_name and bf
    as for report().  Per genome, ascending by name, one nts_bf_sample_intervals call over its gaps only (sample_gaps; `sampling`:
    its result at this rate, where the caller has it already), then one nts_iv_links over all of them on ctx: a hash no genome has
    twice among its sampled gap k-mers is an anchor of every two gaps that have it, and two gaps with at least min_anchors anchors
    are a link.  Returns one dict per link with LINK_COLUMNS' keys, in the join's order: by genome a, gap a, genome b, gap b (a
    before b in the order of the names)."""
    if rate < 1 or min_anchors < 1:
        raise ValueError("links: rate and min_anchors must be at least 1")
    names = sorted(genomes_by_name)
    rows_of = {name: [r for r in gap_rows if r["genome"] == name] for name in names}
    lists, sampled = sampling if sampling is not None else sample_gaps(genomes_by_name, bf, k, gap_rows, rate)
    out = []
    for ln in ctx.iv_links(lists, min_anchors):
        la, lb = int(ln["list_a"]), int(ln["list_b"])
        a, b = rows_of[names[la]][int(ln["iv_a"])], rows_of[names[lb]][int(ln["iv_b"])]
        row = {"anchors": int(ln["anchors"]), "orientation": orientation(int(ln["fwd"]), int(ln["rev"])), "placement": placement(a, b)}
        for x, r, lst in (("a", a, la), ("b", b, lb)):
            row.update({f"genome_{x}": r["genome"], f"contig_{x}": r["contig"], f"start_{x}": r["start"], f"end_{x}": r["end"],
                        f"left_{x}": r["left_block"], f"right_{x}": r["right_block"], f"from_{x}": r["start"] + int(ln[f"min_off_{x}"]),
                        f"to_{x}": r["start"] + int(ln[f"max_off_{x}"]) + int(k), f"sampled_{x}": int(sampled[lst][int(ln[f"iv_{x}"])])})
        out.append(row)
    return out


def links_table(rows, k, rate, min_anchors, bits):
    "<prefix>.gap_links.tsv: a header, one line per link (links()' rows, in their order), then `# k K, rate R, min_anchors M, filter BITS bits`"
    lines = ["\t".join(LINK_COLUMNS)]
    for r in rows:
        lines.append("\t".join(str(r[c]) for c in LINK_COLUMNS))
    lines.append(f"# k {int(k)}, rate {int(rate)}, min_anchors {int(min_anchors)}, filter {int(bits)} bits")
    return "\n".join(lines) + "\n"


def blocks_in_span(blocks, genome, contig, a, b):
    "the ids of the table's blocks (assess.read_blocks' rows) whose interval on `contig` of `genome` intersects [a, b): file order, each once"
    ids = []
    for r in blocks:
        if r.genome == genome and r.contig == contig and r.start < b and r.end > a and r.block_id not in ids:
            ids.append(r.block_id)
    return ids


def block_placement(gap, target_genome, ids):
    """of a gap's link into a block interval: `own` when the interval is the gap's own genome's -- a second copy of sequence the genome
    has inside a block --; otherwise `flank` when the blocks the anchors span (ids) include the gap's left or right block -- sequence
    the neighbouring block covers in the other genome --; `other` otherwise -- it lies in a block elsewhere"""
    if target_genome == gap["genome"]:
        return "own"
    flanks = {gap["left_block"], gap["right_block"]} - {"."}
    return "flank" if flanks & set(ids) else "other"


def gap_to_block(found, n):
    "of the links of the 2n lists (n lists of gaps, then n of block intervals: a LINK_DTYPE array), those of a gap and a block interval, in their order"
    return found[(found["list_a"] < n) & (found["list_b"] >= n)]


def block_links(ctx, genomes_by_name, bf, k, gap_rows, block_rows, blocks, lists, sampled, rate=LINKS_RATE, min_anchors=LINKS_MIN):
    """where the gaps' sampled k-mers occur inside the blocks of every genome, the gap's own included.  gap_rows, block_rows: report()'s
    (block_rows = the merged in-block intervals); blocks: assess.read_blocks' rows; lists, sampled: sample_gaps() at this rate.  The
    hashes of all lists become one exact set on the GPU (nts_hset_build); per genome, ascending by name, one
    nts_hset_sample_intervals call over its merged intervals writes the k-mers under the threshold whose hash is in the set (every
    member is held by the filter, so bf is not probed; a genome given as a loader is loaded once more and freed after its sweep);
    one nts_iv_links over the 2n lists -- a hash is usable when none of them has it twice --, of which the links of a gap and a
    block interval are kept.  Returns (rows, hashes in the set): one dict per link with BLOCK_LINK_COLUMNS' keys, by gap genome, gap,
    target genome, target interval."""
    import numpy as np
    from .device import HashSet
    if rate < 1 or min_anchors < 1:
        raise ValueError("block_links: rate and min_anchors must be at least 1")
    names = sorted(genomes_by_name)
    n = len(names)
    if n > MAX_BLOCK_LINK_GENOMES:
        raise ValueError(f"block_links: {n} genomes; at most {MAX_BLOCK_LINK_GENOMES} (the join takes 64 lists: every genome's gaps and its blocks)")
    gaps_of = {name: [r for r in gap_rows if r["genome"] == name] for name in names}
    merged_of = {name: [r for r in block_rows if r["genome"] == name] for name in names}
    members = np.unique(np.concatenate([np.asarray(lst["h0"], dtype=np.uint64) for lst in lists] + [np.zeros(0, dtype=np.uint64)]))
    hset = HashSet(ctx, members)
    hits, hit_counts = [], []
    try:
        def sweep(name, g):
            rec, counts = g.hset_sample_intervals(hset, _interval_rows(g, merged_of[name]), k, rate)
            hits.append(rec)
            hit_counts.append(counts)
        _each_genome(genomes_by_name, names, sweep)
    finally:
        hset.free()
    out = []
    for ln in gap_to_block(ctx.iv_links(list(lists) + hits, min_anchors), n):
        la, lt = int(ln["list_a"]), int(ln["list_b"]) - n
        gap, target = gaps_of[names[la]][int(ln["iv_a"])], merged_of[names[lt]][int(ln["iv_b"])]
        from_t, to_t = target["start"] + int(ln["min_off_b"]), target["start"] + int(ln["max_off_b"]) + int(k)
        ids = blocks_in_span(blocks, target["genome"], target["contig"], from_t, to_t)
        row = {c: gap[c] for c in ("genome", "contig", "start", "end", "left_block", "right_block")}
        row.update({"target_genome": target["genome"], "target_contig": target["contig"], "target_start": target["start"], "target_end": target["end"],
                    "blocks": ",".join(ids), "anchors": int(ln["anchors"]), "orientation": orientation(int(ln["fwd"]), int(ln["rev"])),
                    "from": gap["start"] + int(ln["min_off_a"]), "to": gap["start"] + int(ln["max_off_a"]) + int(k), "from_t": from_t, "to_t": to_t,
                    "sampled": int(sampled[la][int(ln["iv_a"])]), "target_hits": int(hit_counts[lt][int(ln["iv_b"])]),
                    "placement": block_placement(gap, target["genome"], ids)})
        out.append(row)
    return out, int(members.size)


def block_links_table(rows, k, rate, min_anchors, bits, n_set):
    """<prefix>.gap_block_links.tsv: a header, one line per link (block_links()' rows, in their order), then
    `# k K, rate R, min_anchors M, filter BITS bits, set N hashes`"""
    lines = ["\t".join(BLOCK_LINK_COLUMNS)]
    for r in rows:
        lines.append("\t".join(str(r[c]) for c in BLOCK_LINK_COLUMNS))
    lines.append(f"# k {int(k)}, rate {int(rate)}, min_anchors {int(min_anchors)}, filter {int(bits)} bits, set {int(n_set)} hashes")
    return "\n".join(lines) + "\n"


def copy_stats(counts, own):
    """a gap's line of <prefix>.gap_copies.tsv from its count matrix: counts[t][j] = how often genome t holds the hash of the gap's
    j-th sampled record, genome-wide (records, not distinct hashes: a hash the gap has twice has two columns); own = the row of the
    gap's own genome.  sampled = m, the records; single_own: those its own genome holds exactly once; single_all: those every genome
    holds exactly once; absent_some: those some genome does not hold (the common filter let them through: a false positive);
    copies_own_median / copies_own_max: the lower median and the maximum of the own genome's counts; copies_any_median: the lower
    median of the largest count over the genomes; class: `unique` when more than half of the records are single_all -- the chaining
    could have used the gap: look at the thresholds --, else `repeat` when more than half are not single_own -- the graph stage drops
    what a genome has twice, no threshold brings it back --, else `mixed`.  Without records the last five are None and the class `.`."""
    import numpy as np
    c = np.asarray(counts, dtype=np.int64)
    c = c.reshape(c.shape[0], -1) if c.ndim == 2 else c.reshape(0, 0)
    m = int(c.shape[1]) if c.shape[0] else 0
    if m == 0:
        return {"sampled": 0, "single_own": 0, "single_all": 0, "absent_some": None, "copies_own_median": None, "copies_own_max": None,
                "copies_any_median": None, "class": "."}
    mine = c[own]
    single_own, single_all = int((mine == 1).sum()), int((c == 1).all(axis=0).sum())
    kind = "unique" if 2 * single_all > m else "repeat" if 2 * (m - single_own) > m else "mixed"
    return {"sampled": m, "single_own": single_own, "single_all": single_all, "absent_some": int((c == 0).any(axis=0).sum()),
            "copies_own_median": int(np.sort(mine)[(m - 1) // 2]), "copies_own_max": int(mine.max()),
            "copies_any_median": int(np.sort(c.max(axis=0))[(m - 1) // 2]), "class": kind}


def count_genomes(ctx, genomes_by_name, k, lists, rate=LINKS_RATE, sites=None):
    """the device side of copies() and copy_sites(): the distinct hashes of all lists become one exact set and one table of counts on
    the GPU; per genome, ascending by name: clear, one nts_hset_count_intervals call over the WHOLE genome -- one interval per record
    --, the counts of the set read back by hash (a genome given as a loader is loaded once and freed after its sweeps; the filter is
    not probed: every member is held by it).  sites = (cap, step, min_hits): behind a genome's counts, while they are still in the
    table, one nts_hset_sample_intervals_capped call over the same intervals writes where the members with a count in 1..cap occur
    -- at most members * cap records of 16 bytes -- and one nts_iv_sites call joins the lists against them.  Returns (members,
    matrix, found): the sorted distinct hashes, matrix[t][i] = how often genome t holds members[i], and per genome (record names,
    SITE_DTYPE array) -- None without `sites`."""
    import numpy as np
    from .device import HashCounts, HashSet
    names = sorted(genomes_by_name)
    members = np.unique(np.concatenate([np.asarray(lst["h0"], dtype=np.uint64) for lst in lists] + [np.zeros(0, dtype=np.uint64)]))
    hset = HashSet(ctx, members)
    per_genome, found = [], []
    try:
        counts = HashCounts(ctx, hset)
        try:
            def sweep(name, g):
                whole = [(j, 0, int(n)) for j, n in enumerate(g.rec_len)]
                counts.clear()
                g.hset_count_intervals(hset, counts, whole, k, rate)
                per_genome.append(counts.read(members))
                if sites is not None:
                    cap, step, min_hits = sites
                    occurrences, _ = g.hset_sample_intervals_capped(hset, counts, cap, whole, k, rate)
                    found.append((list(g.names), ctx.iv_sites(lists, occurrences, step, min_hits)))
            _each_genome(genomes_by_name, names, sweep)
        finally:
            counts.free()
    finally:
        hset.free()
    matrix = np.stack(per_genome).astype(np.int64) if per_genome else np.zeros((0, members.size), dtype=np.int64)
    return members, matrix, (found if sites is not None else None)


def _gap_counts(names, gap_rows, lists, sampled, members, matrix, who):
    "(list index, gap index, gap row, counts[genome][record], the records' hashes) per gap, in gap_rows' order"
    import numpy as np
    gaps_of = {name: [r for r in gap_rows if r["genome"] == name] for name in names}
    for li, name in enumerate(names):
        h0 = np.asarray(lists[li]["h0"], dtype=np.uint64)
        of_records = matrix[:, np.searchsorted(members, h0)]                    # [genome, record]
        ends = np.concatenate(([0], np.cumsum(np.asarray(sampled[li], dtype=np.int64))))
        if len(sampled[li]) != len(gaps_of[name]) or int(ends[-1]) != h0.size:
            raise ValueError(f"{who}: the sampling of {name} is not that of these gaps")
        for q, gap in enumerate(gaps_of[name]):
            a, b = int(ends[q]), int(ends[q + 1])
            yield li, q, gap, of_records[:, a:b], h0[a:b]


def copies(ctx, genomes_by_name, k, gap_rows, lists, sampled, rate=LINKS_RATE, counted=None):
    """how often each genome holds each gap's sampled k-mers, genome-wide.  gap_rows: report()'s; lists, sampled: sample_gaps() at
    this rate (one sampling serves links(), block_links() and this).  The distinct hashes of all lists become one exact set and one
    table of counts on the GPU; per genome, ascending by name: clear, one nts_hset_count_intervals call over the WHOLE genome -- one
    interval per record --, the counts of the set read back by hash (count_genomes; `counted`: its result for these lists at this
    rate, where the caller has it already -- one count sweep per genome serves this and copy_sites()).  Returns (rows, hashes in the
    set, absent, sampled): one dict per gap with COPY_COLUMNS' keys (copy_stats), in gap_rows' order; absent = the sampled records some genome does not hold at all, of
    `sampled` records in all -- the filter's false positives among them, counted.  A gap's own genome must hold each of the gap's
    hashes at least as often as the gap's records do: anything else is a fault of the device code and raises."""
    import numpy as np
    if rate < 1:
        raise ValueError("copies: rate must be at least 1")
    names = sorted(genomes_by_name)
    members, matrix, _ = counted if counted is not None else count_genomes(ctx, genomes_by_name, k, lists, rate)
    out, absent, total = [], 0, 0
    for li, _, gap, sub, h0 in _gap_counts(names, gap_rows, lists, sampled, members, matrix, "copies"):
        _, inverse, times = np.unique(h0, return_inverse=True, return_counts=True)
        if (sub[li] < times[inverse]).any():
            raise RuntimeError(f"copies: {names[li]} {gap['contig']}:{gap['start']}-{gap['end']}: the genome-wide count of a sampled k-mer is below "
                               "its count inside the gap (device counts are wrong)")
        row = {c: gap[c] for c in ("genome", "contig", "start", "end", "left_block", "right_block")}
        row.update(copy_stats(sub, li))
        absent += row["absent_some"] or 0
        total += row["sampled"]
        out.append(row)
    return out, int(members.size), absent, total


def copies_table(rows, k, rate, bits, n_set, absent_total, sampled_total):
    """<prefix>.gap_copies.tsv: a header, one line per gap (copies()' rows: the gaps of <prefix>.gaps.tsv, in its order; NA where a gap
    has no sampled k-mer), then `# k K, rate R, filter BITS bits, set N hashes, absent A of T sampled`"""
    lines = ["\t".join(COPY_COLUMNS)]
    for r in rows:
        lines.append("\t".join("NA" if r[c] is None else str(r[c]) for c in COPY_COLUMNS))
    lines.append(f"# k {int(k)}, rate {int(rate)}, filter {int(bits)} bits, set {int(n_set)} hashes, absent {int(absent_total)} of {int(sampled_total)} sampled")
    return "\n".join(lines) + "\n"


def site_placement(gap, target_genome, target_contig, from_t, to_t):
    """of a site [from_t, to_t) on `target_contig` of `target_genome`, seen from the gap (a row with genome, contig, start, end):
    `self` when it lies on the gap's own contig and intersects the gap -- the gap's k-mers found where they were taken --; `own` when
    the target is the gap's own genome otherwise -- another copy in that genome --; `other` when it is another genome"""
    if target_genome != gap["genome"]:
        return "other"
    if target_contig == gap["contig"] and from_t < gap["end"] and to_t > gap["start"]:
        return "self"
    return "own"


def site_usable(counts, cap):
    """from a gap's count matrix (counts[t][j] = how often genome t holds the hash of the gap's j-th sampled record): ([per genome t,
    the records usable against it: 1 <= counts[t][j] <= cap], the (record, genome) pairs over the cap)"""
    import numpy as np
    c = np.asarray(counts, dtype=np.int64)
    c = c.reshape(c.shape[0], -1) if c.ndim == 2 else c.reshape(0, 0)
    return [int(x) for x in ((c >= 1) & (c <= int(cap))).sum(axis=1)], int((c > int(cap)).sum())


def copy_sites(ctx, genomes_by_name, k, gap_rows, blocks, lists, sampled, rate=LINKS_RATE, cap=SITES_CAP, step=SITES_STEP, min_hits=LINKS_MIN, counted=None):
    """where each genome, the gap's own included, holds the gaps' sampled k-mers close together.  gap_rows: report()'s; blocks:
    assess.read_blocks' rows; lists, sampled: sample_gaps() at this rate; counted: count_genomes(..., sites=(cap, step, min_hits)) for
    these lists where the caller has it already (one count sweep per genome serves copies() and this), else it is run here.  A hash of
    a gap is usable against genome t when t holds it 1..cap times; the occurrences of the usable hashes in t, paired with the gap's
    records of the same hash, ordered by (record, position, the record's place in its list), fall into sites: maximal runs within one
    record whose consecutive positions differ by at most `step`; a site with at least min_hits pairs is kept.  Returns (rows, hashes
    in the set, over_cap, of): one dict per gap and site with SITE_COLUMNS' keys, by gap genome, gap, target genome, target record,
    from_t; over_cap = the (sampled record, genome) pairs whose count is above the cap, of `of` = records * genomes.  When the pairs
    of one target reach 2^32 the join refuses the call and this raises with its message."""
    if rate < 1 or cap < 1 or step < 0 or min_hits < 1:
        raise ValueError("copy_sites: rate, cap and min_hits must be at least 1, step at least 0")
    names = sorted(genomes_by_name)
    members, matrix, found = counted if counted is not None else count_genomes(ctx, genomes_by_name, k, lists, rate, sites=(cap, step, min_hits))
    if found is None:
        raise ValueError("copy_sites: `counted` was made without sites")
    facts, over_cap, total = {}, 0, 0                            # (list, gap) -> (gap row, class, sampled, usable per genome)
    for li, q, gap, sub, _ in _gap_counts(names, gap_rows, lists, sampled, members, matrix, "copy_sites"):
        usable, over = site_usable(sub, cap)
        facts[(li, q)] = (gap, copy_stats(sub, li)["class"], int(sub.shape[1]), usable)
        over_cap += over
        total += int(sub.shape[1]) * len(names)
    keyed = []
    for ti, (contigs, sites) in enumerate(found):
        for s in sites:
            keyed.append(((int(s["list_q"]), int(s["iv_q"]), ti, int(s["rec_t"]), int(s["first_t"])), contigs, s))
    keyed.sort(key=lambda t: t[0])
    out = []
    for (li, q, ti, _, _), contigs, s in keyed:
        gap, kind, m, usable = facts[(li, q)]
        contig, from_t, to_t = contigs[int(s["rec_t"])], int(s["first_t"]), int(s["last_t"]) + int(k)
        row = {c: gap[c] for c in ("genome", "contig", "start", "end", "left_block", "right_block")}
        row.update({"class": kind, "target_genome": names[ti], "target_contig": contig, "from_t": from_t, "to_t": to_t,
                    "blocks": ",".join(blocks_in_span(blocks, names[ti], contig, from_t, to_t)) or ".", "hits": int(s["hits"]),
                    "orientation": orientation(int(s["fwd"]), int(s["rev"])), "from": gap["start"] + int(s["min_off_q"]),
                    "to": gap["start"] + int(s["max_off_q"]) + int(k), "sampled": m, "usable": usable[ti],
                    "placement": site_placement(gap, names[ti], contig, from_t, to_t)})
        out.append(row)
    return out, int(members.size), over_cap, total


def copy_sites_table(rows, k, rate, cap, step, min_hits, bits, n_set, over_cap, of_total):
    """<prefix>.gap_copy_sites.tsv: a header, one line per gap and site (copy_sites()' rows, in their order), then
    `# k K, rate R, cap C, step D, min_hits M, filter BITS bits, set N hashes, over_cap X of Y`"""
    lines = ["\t".join(SITE_COLUMNS)]
    for r in rows:
        lines.append("\t".join(str(r[c]) for c in SITE_COLUMNS))
    lines.append(f"# k {int(k)}, rate {int(rate)}, cap {int(cap)}, step {int(step)}, min_hits {int(min_hits)}, filter {int(bits)} bits, "
                 f"set {int(n_set)} hashes, over_cap {int(over_cap)} of {int(of_total)}")
    return "\n".join(lines) + "\n"


def sample_all(genomes_by_name, k, gap_rows, rate=LINKS_RATE):
    """(lists, sampled): sample_gaps() without a filter -- per genome, ascending by name, the records and the per-gap counts of one
    nts_sample_intervals call over its gaps only: every valid k-mer wholly inside a gap with h0 <= (2^64 - 1) // rate, whatever holds
    it.  A k-mer that recurs is sampled at every recurrence or at none."""
    if rate < 1:
        raise ValueError("sample_all: rate must be at least 1")
    lists, sampled = [], []

    def sweep(name, g):
        rec, counts = g.sample_intervals(_interval_rows(g, [r for r in gap_rows if r["genome"] == name]), k, rate)
        lists.append(rec)
        sampled.append(counts)
    _each_genome(genomes_by_name, sorted(genomes_by_name), sweep)
    return lists, sampled


def period_row(gap, k, sampled, result, min_hits):
    """a gap's line of <prefix>.gap_periods.tsv: gap = its row (genome, contig, start, end, kind); sampled = its unfiltered records;
    result = its (recurring, period, period_hits, first_off, last_off) of nts_iv_periods.  from / to = the stretch the records at the
    period cover, one unit before the first of them to the end of the last; copies = covered / period in tenths, rounded down;
    class: `.` below min_hits records at the period (period, from, to, copies and covered_fraction are then None), else `tandem` when
    the stretch is more than half of the gap, else `partial`.  Integer arithmetic throughout."""
    recurring, period, hits, first_off, last_off = (int(x) for x in result)
    length = gap["end"] - gap["start"]
    row = {c: gap[c] for c in ("genome", "contig", "start", "end", "kind")}
    row.update({"length": length, "sampled": int(sampled), "recurring": recurring, "period_hits": hits})
    if hits < int(min_hits) or period < 1:
        row.update({"period": None, "from": None, "to": None, "copies": None, "covered_fraction": None, "class": "."})
        return row
    lo, hi = gap["start"] + first_off, gap["start"] + last_off + int(k)
    covered = hi - lo
    tenths = (10 * covered) // period
    row.update({"period": period, "from": lo, "to": hi, "copies": f"{tenths // 10}.{tenths % 10}", "covered_fraction": _ratio(covered / length),
                "class": "tandem" if 2 * covered > length else "partial"})
    return row


def periods(ctx, genomes_by_name, k, gap_rows, rate=LINKS_RATE, min_hits=LINKS_MIN, sampling=None, with_sampling=False):
    """which gaps are tandem arrays: gap_rows are report()'s (every genome's, in its order); genomes_by_name as for report().  Per
    genome, ascending by name, one nts_sample_intervals call over its gaps (sample_all: a genome given as a loader is loaded once and
    freed after its sweep), then one nts_iv_periods call on ctx over that genome's records.  Returns one dict per gap with
    PERIOD_COLUMNS' keys (period_row), in gap_rows' order.  2^32 records of one genome or more: the call refuses and this raises with
    its message (raise the rate).  sampling: sample_all()'s result at this rate, where the caller has it already; with_sampling: return
    (rows, sampling) -- one sample_all serves this and families()."""
    if rate < 1 or min_hits < 1:
        raise ValueError("periods: rate and min_hits must be at least 1")
    names = sorted(genomes_by_name)
    lists, sampled = sampling if sampling is not None else sample_all(genomes_by_name, k, gap_rows, rate)
    out = []
    for li, name in enumerate(names):
        mine = [r for r in gap_rows if r["genome"] == name]
        if len(sampled[li]) != len(mine):
            raise ValueError(f"periods: the sampling of {name} is not that of these gaps")
        found = ctx.iv_periods(lists[li], len(mine))
        for q, gap in enumerate(mine):
            out.append(period_row(gap, k, int(sampled[li][q]), tuple(int(found[q][c]) for c in ("recurring", "period", "period_hits", "first_off", "last_off")),
                                  min_hits))
    return (out, (lists, sampled)) if with_sampling else out


def periods_table(rows, k, rate, min_hits):
    "<prefix>.gap_periods.tsv: a header, one line per gap (periods()' rows: the gaps of <prefix>.gaps.tsv, in its order; `.` where a gap has no period), then `# k K, rate R, min_hits M`"
    lines = ["\t".join(PERIOD_COLUMNS)]
    for r in rows:
        lines.append("\t".join("." if r[c] is None else str(r[c]) for c in PERIOD_COLUMNS))
    lines.append(f"# k {int(k)}, rate {int(rate)}, min_hits {int(min_hits)}")
    return "\n".join(lines) + "\n"


def family_row(period_row_, family, members, genomes, array_hashes, shared_hashes):
    """an array's line of <prefix>.gap_families.tsv: period_row_ = its row of periods() (class `tandem` or `partial`); family = its
    family's number (1, 2, ... by the smallest array index); members = the arrays of the family, genomes = the genomes that have one;
    array_hashes = the distinct hashes that carry the array's period, shared_hashes = those of them another array also holds"""
    row = {c: period_row_[c] for c in ("genome", "contig", "start", "end", "length", "kind", "period", "class")}
    row.update({"family": int(family), "members": int(members), "genomes": int(genomes), "array_hashes": int(array_hashes),
                "shared_hashes": int(shared_hashes)})
    return row


def family_site_placement(genome, contig, from_, to, member_gaps, gap_rows):
    """of a family's site [from_, to) on `contig` of `genome`, by precedence: `array` when it intersects a gap that is a member array of
    its family (member_gaps: those gaps' rows), `gap` when it intersects any other gap (gap_rows: every gap's row), `block` otherwise"""
    def hit(rows):
        return any(r["genome"] == genome and r["contig"] == contig and from_ < r["end"] and to > r["start"] for r in rows)
    return "array" if hit(member_gaps) else "gap" if hit(gap_rows) else "block"


def family_site_row(family, genome, contig, first, last, hits, k, period, period_hits, min_hits, block_ids, placement_):
    """a site's line of <prefix>.gap_family_sites.tsv: first / last = its first and last position (from = first, to = last + k);
    period, period_hits = nts_iv_periods' over the site's own occurrences; copies = (10 * (to - from)) // period in tenths, rounded
    down; with period_hits < min_hits the three read None.  block_ids: blocks_in_span of the site.  Integer arithmetic throughout."""
    from_, to = int(first), int(last) + int(k)
    row = {"family": int(family), "genome": genome, "contig": contig, "from": from_, "to": to, "length": to - from_, "hits": int(hits),
           "blocks": ",".join(block_ids) or ".", "placement": placement_}
    if int(period_hits) < int(min_hits) or int(period) < 1:
        row.update({"period": None, "period_hits": None, "copies": None})
    else:
        tenths = (10 * (to - from_)) // int(period)
        row.update({"period": int(period), "period_hits": int(period_hits), "copies": f"{tenths // 10}.{tenths % 10}"})
    return row


def _site_records(occurrences, hashes, hash_family, sites):
    """the occurrences that lie in a kept site, as records for nts_iv_periods: iv = the site's index in `sites` (FSITE_DTYPE, in
    (family, rec, first) order), off = position - the site's first position; in (iv, off) order"""
    import numpy as np
    from .device import SAMPLE_DTYPE
    out = np.zeros(0, dtype=SAMPLE_DTYPE)
    if not len(sites) or not len(occurrences):
        return out
    at = np.searchsorted(hashes, occurrences["h0"])
    member = (at < hashes.size) & (hashes[np.minimum(at, hashes.size - 1)] == occurrences["h0"])
    occ = occurrences[member]
    fam = hash_family[at[member]].astype(np.uint64)
    order = np.argsort(fam, kind="stable")                      # (family, rec, off): the input order supplies the rest
    occ, fam = occ[order], fam[order]
    key_o = (fam << np.uint64(32)) | occ["iv"].astype(np.uint64)
    key_s = (sites["family"].astype(np.uint64) << np.uint64(32)) | sites["rec"].astype(np.uint64)
    _, rank = np.unique(np.concatenate([key_s, key_o]), return_inverse=True)
    rank = rank.astype(np.uint64)
    place_s = (rank[:key_s.size] << np.uint64(32)) | sites["first"].astype(np.uint64)
    place_o = (rank[key_s.size:] << np.uint64(32)) | occ["off"].astype(np.uint64)
    j = np.searchsorted(place_s, place_o, side="right").astype(np.int64) - 1
    jj = np.maximum(j, 0)
    inside = (j >= 0) & (key_s[jj] == key_o) & (occ["off"] <= sites["last"][jj])
    out = np.zeros(int(inside.sum()), dtype=SAMPLE_DTYPE)
    out["h0"], out["iv"], out["off"] = occ["h0"][inside], jj[inside], occ["off"][inside] - sites["first"][jj[inside]]
    return out


def families(ctx, genomes_by_name, k, gap_rows, blocks, period_rows, rate=LINKS_RATE, min_hits=LINKS_MIN, step=SITES_STEP, sampling=None):
    """which tandem arrays are the same satellite, and where each genome holds it.  gap_rows: report()'s; blocks: assess.read_blocks'
    rows; period_rows: periods()' at this rate and min_hits, one per gap in gap_rows' order -- a gap whose class is `tandem` or
    `partial` is an array, numbered 0, 1, ... in that order; sampling: sample_all()'s at this rate where the caller has it (periods(...,
    with_sampling=True)), else taken here.  Per genome one nts_iv_period_hashes call reduces its arrays to the distinct hashes that
    carry their periods; one nts_iv_families joins the arrays that share a hash; the hashes become one exact set (nts_hset_build) and
    per genome, ascending by name (a loader is loaded once and freed after its sweep): one nts_hset_sample_intervals over the WHOLE
    genome, one nts_iv_family_sites, one nts_iv_periods on the kept sites.  Returns (rows, site rows, hashes in the set): one dict per
    array with FAMILY_COLUMNS' keys, in array order, and one per kept site with FAMILY_SITE_COLUMNS' keys, by (family, genome,
    record, from).  A record of 2^32 bases, or 2^32 occurrences in one genome: the call refuses and this raises with its message."""
    import numpy as np
    from .device import SAMPLE_DTYPE, HashSet
    if rate < 1 or min_hits < 1 or step < 0:
        raise ValueError("families: rate and min_hits must be at least 1, step at least 0")
    if len(period_rows) != len(gap_rows):
        raise ValueError("families: one period row per gap")
    names = sorted(genomes_by_name)
    lists, sampled = sampling if sampling is not None else sample_all(genomes_by_name, k, gap_rows, rate)
    arrays = [i for i, r in enumerate(period_rows) if r["class"] in ("tandem", "partial")]
    index_of = {i: a for a, i in enumerate(arrays)}            # gap (its place in gap_rows) -> array
    parts = []
    for li, name in enumerate(names):
        mine = [i for i, r in enumerate(gap_rows) if r["genome"] == name]
        if len(sampled[li]) != len(mine):
            raise ValueError(f"families: the sampling of {name} is not that of these gaps")
        period = np.array([period_rows[i]["period"] if i in index_of else 0 for i in mine], dtype=np.uint32)
        if not period.any():
            continue
        found = ctx.iv_period_hashes(lists[li], len(mine), period)
        found["iv"] = np.array([index_of.get(i, 0) for i in mine], dtype=np.uint32)[found["iv"]]
        parts.append(found)
    pairs = np.concatenate(parts) if parts else np.zeros(0, dtype=SAMPLE_DTYPE)
    family, hashes, hash_family = ctx.iv_families(pairs, len(arrays))
    number = {int(root): n + 1 for n, root in enumerate(sorted(set(family.tolist())))}       # by the smallest array index
    _, inverse, holders = np.unique(pairs["h0"], return_inverse=True, return_counts=True)      # (pairs are distinct: holders = arrays)
    rows = []
    for a, i in enumerate(arrays):
        of_family = [b for b in range(len(arrays)) if family[b] == family[a]]
        mine = pairs["iv"] == a
        rows.append(family_row(period_rows[i], number[int(family[a])], len(of_family), len({period_rows[arrays[b]]["genome"] for b in of_family}),
                               int(mine.sum()), int((holders[inverse[mine]] > 1).sum())))
    site_rows = []
    if hashes.size:
        numbered = np.array([number[int(f)] for f in hash_family], dtype=np.uint32)
        member_gaps = {}
        for a, i in enumerate(arrays):
            member_gaps.setdefault(number[int(family[a])], []).append(gap_rows[i])
        hset = HashSet(ctx, hashes)
        try:
            def sweep(name, g):
                whole = [(j, 0, int(n)) for j, n in enumerate(g.rec_len)]
                occurrences, _ = g.hset_sample_intervals(hset, whole, k, rate)
                sites = ctx.iv_family_sites(occurrences, hashes, numbered, step, min_hits)
                found = ctx.iv_periods(_site_records(occurrences, hashes, numbered, sites), len(sites))
                contigs = list(g.names)
                for s, p in zip(sites, found):
                    contig, from_, to = contigs[int(s["rec"])], int(s["first"]), int(s["last"]) + int(k)
                    site_rows.append(family_site_row(int(s["family"]), name, contig, from_, int(s["last"]), int(s["hits"]), k, int(p["period"]),
                                                     int(p["period_hits"]), min_hits, blocks_in_span(blocks, name, contig, from_, to),
                                                     family_site_placement(name, contig, from_, to, member_gaps[int(s["family"])], gap_rows)))
            _each_genome(genomes_by_name, names, sweep)
        finally:
            hset.free()
        site_rows.sort(key=lambda r: r["family"])               # stable: genomes by name, then (record, from) within a family
    return rows, site_rows, int(hashes.size)


def _families_footer(k, rate, min_hits, step, n_arrays, n_families, n_set):
    return (f"# k {int(k)}, rate {int(rate)}, min_hits {int(min_hits)}, step {int(step)}, arrays {int(n_arrays)}, families {int(n_families)}, "
            f"set {int(n_set)} hashes")


def families_table(rows, k, rate, min_hits, step, n_set):
    """<prefix>.gap_families.tsv: a header, one line per array (families()' rows, in their order), then
    `# k K, rate R, min_hits M, step D, arrays A, families F, set N hashes`"""
    lines = ["\t".join(FAMILY_COLUMNS)]
    for r in rows:
        lines.append("\t".join(str(r[c]) for c in FAMILY_COLUMNS))
    lines.append(_families_footer(k, rate, min_hits, step, len(rows), len({r["family"] for r in rows}), n_set))
    return "\n".join(lines) + "\n"


def family_sites_table(site_rows, k, rate, min_hits, step, n_arrays, n_families, n_set):
    """<prefix>.gap_family_sites.tsv: a header, one line per kept site (families()' site rows, in their order; `.` where a site has no
    period), then the footer of families_table()"""
    lines = ["\t".join(FAMILY_SITE_COLUMNS)]
    for r in site_rows:
        lines.append("\t".join("." if r[c] is None else str(r[c]) for c in FAMILY_SITE_COLUMNS))
    lines.append(_families_footer(k, rate, min_hits, step, n_arrays, n_families, n_set))
    return "\n".join(lines) + "\n"


def build_parser():
    "bin/ntsynt_gaps' options"
    import argparse
    p = argparse.ArgumentParser(prog="ntsynt_gaps", description="What the synteny blocks of a finished run leave out: every gap of every genome "
                                "with its N bases and the share of its k-mers that the run's common Bloom filter holds (GPU)")
    p.add_argument("--tsv", help="synteny block table (<prefix>.synteny_blocks.tsv)", required=True)
    p.add_argument("--fastas", help="the compared genomes (matched to column 2 of the table by base name)", nargs="+", required=True)
    p.add_argument("--common", help="the run's common Bloom filter (<prefix>.common.bf); k is read from its header", required=True)
    p.add_argument("--out", help="file for the per-gap table [stdout]")
    p.add_argument("--summary-out", help="file for the per-genome summary [stdout, after the table]")
    p.add_argument("--links-out", help="also write the links between the gaps of different genomes to this file (<prefix>.gap_links.tsv)")
    p.add_argument("--block-links-out", help="also write the links between the gaps and the block intervals of every genome, the gap's own included, "
                   "to this file (<prefix>.gap_block_links.tsv); uses --links-rate and --links-min")
    p.add_argument("--copies-out", help="also write how often each genome holds each gap's sampled k-mers, genome-wide, and the gap's class "
                   "(unique / repeat / mixed) to this file (<prefix>.gap_copies.tsv); uses --links-rate")
    p.add_argument("--copy-sites-out", help="also write where each genome, the gap's own included, holds each gap's sampled k-mers close together "
                   "(the copies of a repeat gap) to this file (<prefix>.gap_copy_sites.tsv); uses --links-rate and --links-min")
    p.add_argument("--periods-out", help="also write, per gap, the period, the copy count and the extent of a tandem array in it, from an unfiltered "
                   "sample of its k-mers, to this file (<prefix>.gap_periods.tsv); uses --links-rate and --links-min")
    p.add_argument("--families-out", help="also write, per tandem array of the periods, its family -- the arrays that share a hash carrying their period -- "
                   "to this file (<prefix>.gap_families.tsv); uses --links-rate, --links-min and --sites-step")
    p.add_argument("--family-sites-out", help="also write where each genome holds each family's k-mers close together, in an array gap, in another gap "
                   "or inside a block, to this file (<prefix>.gap_family_sites.tsv); uses --links-rate, --links-min and --sites-step")
    p.add_argument("--sites-cap", help=f"use a k-mer against a genome that holds it at most this many times [{SITES_CAP}]", type=int, default=SITES_CAP)
    p.add_argument("--sites-step", help=f"two hits of a site lie at most this many bases apart [{SITES_STEP}]", type=int, default=SITES_STEP)
    p.add_argument("--links-rate", help=f"sample one in this many of the gap k-mers the filter holds [{LINKS_RATE}]", type=int, default=LINKS_RATE)
    p.add_argument("--links-min", help=f"anchors a link needs [{LINKS_MIN}]", type=int, default=LINKS_MIN)
    p.add_argument("--device", help="GPU index [0]", type=int, default=0)
    return p


def main(argv=None):
    "bin/ntsynt_gaps"
    import sys
    p = build_parser()
    args = p.parse_args(argv)
    if args.links_rate < 1 or args.links_min < 1:
        p.error("--links-rate and --links-min must be positive")
    if args.sites_cap < 1 or args.sites_cap > 0xFFFFFFFF or args.sites_step < 0 or args.sites_step > 0xFFFFFFFF:
        p.error("--sites-cap must be positive and --sites-step not negative (32-bit values)")
    if args.copy_sites_out and len(args.fastas) > 2 * MAX_BLOCK_LINK_GENOMES:
        p.error(f"--copy-sites-out takes at most {2 * MAX_BLOCK_LINK_GENOMES} genomes")
    if args.block_links_out and len(args.fastas) > MAX_BLOCK_LINK_GENOMES:
        p.error(f"--block-links-out takes at most {MAX_BLOCK_LINK_GENOMES} genomes")
    for path in args.fastas + [args.common, args.tsv]:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Input file {path} not found.")
    from .assess import read_blocks
    from .device import BloomFilter, Context
    from .fasta import basename, read_fasta_device
    from .pipeline import read_bf
    ctx = Context(args.device)
    try:
        bits, k = read_bf(args.common)
        bf = BloomFilter(ctx, bits.size, k)
        bf.from_numpy(bits)
        del bits
        loaders = {basename(path): (lambda path=path: read_fasta_device(ctx, path)[0]) for path in args.fastas}
        try:
            blocks = read_blocks(args.tsv)
            gap_rows, block_rows, n_bits, occupancy = report(ctx, loaders, bf, k, blocks)
            texts = table(gap_rows, k, n_bits, occupancy), summary(gap_rows, block_rows, k, n_bits, occupancy, genomes=list(loaders))
            if args.links_out or args.block_links_out or args.copies_out or args.copy_sites_out:
                sampling = sample_gaps(loaders, bf, k, gap_rows, args.links_rate)
            if args.links_out:
                link_rows = links(ctx, loaders, bf, k, gap_rows, args.links_rate, args.links_min, sampling=sampling)
                with open(args.links_out, "w", encoding="utf-8") as fh:
                    fh.write(links_table(link_rows, k, args.links_rate, args.links_min, n_bits))
            if args.block_links_out:
                b_rows, n_set = block_links(ctx, loaders, bf, k, gap_rows, block_rows, blocks, sampling[0], sampling[1], args.links_rate, args.links_min)
                with open(args.block_links_out, "w", encoding="utf-8") as fh:
                    fh.write(block_links_table(b_rows, k, args.links_rate, args.links_min, n_bits, n_set))
            counted = None                                      # one count sweep per genome serves the copies and the copy sites
            if args.copy_sites_out:
                counted = count_genomes(ctx, loaders, k, sampling[0], args.links_rate, sites=(args.sites_cap, args.sites_step, args.links_min))
                s_rows, n_set, over_cap, of_total = copy_sites(ctx, loaders, k, gap_rows, blocks, sampling[0], sampling[1], args.links_rate, args.sites_cap,
                                                               args.sites_step, args.links_min, counted=counted)
                with open(args.copy_sites_out, "w", encoding="utf-8") as fh:
                    fh.write(copy_sites_table(s_rows, k, args.links_rate, args.sites_cap, args.sites_step, args.links_min, n_bits, n_set, over_cap, of_total))
            if args.copies_out:
                c_rows, n_set, absent, n_sampled = copies(ctx, loaders, k, gap_rows, sampling[0], sampling[1], args.links_rate, counted=counted)
                with open(args.copies_out, "w", encoding="utf-8") as fh:
                    fh.write(copies_table(c_rows, k, args.links_rate, n_bits, n_set, absent, n_sampled))
            if args.periods_out or args.families_out or args.family_sites_out:
                p_rows, unfiltered = periods(ctx, loaders, k, gap_rows, args.links_rate, args.links_min, with_sampling=True)
                if args.periods_out:
                    with open(args.periods_out, "w", encoding="utf-8") as fh:
                        fh.write(periods_table(p_rows, k, args.links_rate, args.links_min))
            if args.families_out or args.family_sites_out:
                f_rows, fs_rows, n_set = families(ctx, loaders, k, gap_rows, blocks, p_rows, args.links_rate, args.links_min, args.sites_step,
                                                  sampling=unfiltered)
                if args.families_out:
                    with open(args.families_out, "w", encoding="utf-8") as fh:
                        fh.write(families_table(f_rows, k, args.links_rate, args.links_min, args.sites_step, n_set))
                if args.family_sites_out:
                    with open(args.family_sites_out, "w", encoding="utf-8") as fh:
                        fh.write(family_sites_table(fs_rows, k, args.links_rate, args.links_min, args.sites_step, len(f_rows),
                                                    len({r["family"] for r in f_rows}), n_set))
        finally:
            bf.free()
    finally:
        ctx.close()
    for text, path in zip(texts, (args.out, args.summary_out)):
        if path:
            with open(path, "w", encoding="utf-8") as fh:
                fh.write(text)
        else:
            sys.stdout.write(text)
    return 0

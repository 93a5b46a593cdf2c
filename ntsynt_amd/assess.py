"""Assessment of a run's synteny blocks (`ntSynt --assess`, bin/ntsynt_block_stats).

Two things, both over `<prefix>.synteny_blocks.tsv`:

* block_stats: the one-line summary of the reference's analysis_scripts/denovo_synteny_block_stats.py (README "Basic assessment of
  synteny blocks"), restated: the same ten columns under the same rules.  Host arithmetic; no GPU, no torch, no numpy.
* block_divergence: the Mash distance of `-d auto` (ntsynt_amd/divergence.py) per block and pair of its genomes, from bottom-s
  sketches of the blocks' intervals taken in one sweep per genome (nts_minhash_intervals) and one pair-count call
  (nts_minhash_pairs); docs/design/04_8_block_assessment.md.
* block_identity (`ntSynt --block-identity`, `ntsynt_block_stats --identity-out`): per block and pair of its lines the exact edit
  distance of the stretches between consecutive anchors -- sampled k-mers either genome has once (nts_sample_intervals,
  nts_iv_anchor_segments, nts_edit_segments); docs/design/04_16_block_identity.md.
* block_variants (`ntSynt --block-variants`, `ntsynt_block_stats --variants-out`): the edits behind those distances -- the canonical
  script of every aligned stretch (nts_edit_script), merged into snv / ins / del events in both genomes' coordinates;
  docs/design/04_17_block_variants.md.
* block_wide_variants (`ntSynt --block-wide-variants`, `ntsynt_block_stats --wide-variants-out`): the same list with the stretches the
  band leaves out included (nts_edit_wide, nts_edit_wide_script), under --identity-max-edits; docs/design/04_19_block_wide_variants.md.
* block_ends (`ntSynt --block-ends`, `ntsynt_block_stats --ends-out`): per block and pair of its lines how far the alignment continues
  in front of the first and behind the last aligned stretch, base for base -- the breakpoints of the pair (nts_edit_extend);
  docs/design/04_20_block_ends.md.
* block end variants (`ntSynt --block-ends --block-end-variants`, `ntsynt_block_stats --ends-out F --end-variants-out G`): the edits
  behind left_edits and right_edits -- the canonical script of every extended flank (nts_edit_extend_script), as snv / ins / del
  events in both genomes' coordinates; docs/design/04_21_block_end_variants.md.
* block MAF (`ntSynt --block-maf`, `ntsynt_block_stats --maf-out`): one pairwise MAF block per PAF record with both aligned rows, made on the
  GPU (nts_cigar_rows); docs/design/04_29_block_maf.md.
* block conservation (`ntSynt --block-conservation`, `ntsynt_block_stats --conservation-out --conservation-stats-out`): per block the runs
  of bases of its first line with one (aligned, match, gap) over the star pairs' CIGARs, made on the GPU (nts_cigar_depth), and the
  covered, core and conserved bases per block; docs/design/04_31_block_conservation.md.
* block variant sites (`ntSynt --block-variant-sites`, `ntsynt_block_stats --variant-sites-out`): per block the reference positions at
  which the other genomes differ, one line per allele with its carriers and one genotype character per row, the bases and the allele
  table made on the GPU (nts_cigar_var_bases, nts_cigar_alleles); docs/design/04_32_block_variant_sites.md.
* block consensus (`ntSynt --block-consensus`, `ntsynt_block_stats --profile-out --consensus-out`): per block one line per variable column
  of its star alignment, insertion columns included, with the tallies of A C G T N and the gap and the plurality call, made on the GPU
  (nts_cigar_profile), and the block's first line with the calls applied; docs/design/04_33_block_consensus.md.
* block chain file (`ntSynt --block-chain`, `ntsynt_block_stats --chain-out`): one UCSC liftover chain per block and pair, the chains of the
  block alignments joined per pair, blocks and data lines made on the GPU (nts_cigar_chain_blocks); docs/design/04_28_block_chain.md.
* block alignments (`ntSynt --block-paf`, `ntsynt_block_stats --paf-out`): one PAF record with a cg:Z: CIGAR per aligned chain of every
  block and pair -- the scripts of all stretches and flanks stitched and run-length merged on the GPU (nts_cigar_build);
  docs/design/04_22_block_alignments.md.  With `--paf-cs` also the cs:Z: tag, both tag texts written on the GPU (nts_cigar_text);
  docs/design/04_26_block_paf_cs.md.
* block lift (`ntSynt --block-lift BED --lift-genome NAME`, `ntsynt_block_stats --lift-bed --lift-genome --lift-out`): the intervals of
  one genome mapped through those alignments into the other genomes -- the coordinate map of the chains' CIGARs on the GPU
  (nts_cigar_lift); docs/design/04_23_block_lift.md.
* lift identity (`ntSynt --lift-identity`, `--lift-windows W`, `ntsynt_block_stats --lift-identity-out`, `--lift-windows --lift-windows-out`):
  the matches, mismatches and missing bases of every lifted interval and of a window grid over one genome -- range sums over the
  chains' CIGARs on the GPU (nts_cigar_lift_stats); docs/design/04_25_lift_identity.md."""
import os
import re
from collections import namedtuple

K_DEFAULT = 21
S_DEFAULT = 1000

STATS_COLUMNS = ("Number_blocks", "Number_blocks_all_asm", "Average_coverage", "Average_coverage_all_asm", "Coverage_min_genome_size",
                 "Average_length", "Median_length", "Total_length", "NG50_length", "N50_length")
DIVERGENCE_COLUMNS = ("block_id", "genome_a", "genome_b", "distance", "shared_hashes", "sketch_size", "kmers_a", "kmers_b")

IDENTITY_K, IDENTITY_RATE, IDENTITY_BAND, IDENTITY_MAX_LEN = 21, 16, 31, 4096
IDENTITY_COLUMNS = ("block_id", "genome_a", "genome_b", "orientation", "length_a", "length_b", "anchors", "segments", "aligned", "aligned_a",
                    "aligned_b", "edits", "identity", "covered_a", "covered_b", "backward", "long", "offband", "invalid", "overband")
ENDS_MAX_LEN, ENDS_MAX_EDITS, ENDS_PENALTY = 4096, 255, 6
ENDS_COLUMNS = ("block_id", "genome_a", "contig_a", "start_a", "end_a", "genome_b", "contig_b", "start_b", "end_b", "orientation", "left_a", "left_b",
                "left_edits", "left_stop", "right_a", "right_b", "right_edits", "right_stop", "ext_start_a", "ext_end_a", "ext_start_b", "ext_end_b")
VARIANT_COLUMNS = ("block_id", "genome_a", "contig_a", "pos_a", "genome_b", "contig_b", "pos_b", "orientation", "type", "length", "seq_a", "seq_b")
END_VARIANT_COLUMNS = VARIANT_COLUMNS[:8] + ("flank",) + VARIANT_COLUMNS[8:]      # (`flank`, left or right, behind `orientation`)
END_VARIANTS_NEED_ENDS = ("the block end variants list the edits of the flanks that the block ends extend and are written from that stage's own pass: "
                          "give --block-ends with --block-end-variants (ntsynt_block_stats: --ends-out with --end-variants-out)")

# one line of a block table (README "Output files"): the block's interval on `contig` of `genome` is [start, end)
BlockRow = namedtuple("BlockRow", ["block_id", "genome", "contig", "start", "end", "strand", "minimizers", "reason"])


def read_blocks(tsv_path):
    "the lines of a synteny block table, in file order"
    rows = []
    with open(tsv_path, "r", encoding="utf-8") as fh:
        for line in fh:
            f = line.strip().split("\t")
            if len(f) < 5:
                continue
            rows.append(BlockRow(f[0], f[1], f[2], int(f[3]), int(f[4]), f[5] if len(f) > 5 else "+", f[6] if len(f) > 6 else "",
                                 f[7] if len(f) > 7 else ""))
    return rows


def genome_sizes(fai_paths):
    """{genome name: sum of the .fai's second column}, in the order given.  The name is the base name of the path in front of its
    `.fai`; a path that does not carry one names no genome (it still counts as an input of the averages)."""
    sizes = {}
    for path in fai_paths:
        m = re.match(r"(\S+).fai", path)
        if not m:
            continue
        total = 0
        with open(path, "r", encoding="utf-8") as fh:
            for line in fh:
                total += int(line.strip().split("\t")[1])
        sizes[os.path.basename(m.group(1))] = total
    return sizes


def _n50(lengths, against):
    "the length at which the lengths, longest first, have summed to half of `against` (0 if they never do)"
    half, run = against * 0.5, 0
    for v in sorted(lengths, reverse=True):
        run += v
        if run >= half:
            return v
    return 0


def _median(lengths):
    v = sorted(lengths)
    mid = len(v) // 2
    return float(v[mid]) if len(v) % 2 else (v[mid - 1] + v[mid]) / 2.0


def block_stats(tsv_path, fai_paths, sizes=None):
    """The reference's de novo statistics of a block table, as a dict keyed by STATS_COLUMNS.  Every figure is taken per genome of the
    table and the per-genome figures are summed and divided by the number of .fai files given; "all_asm" counts the blocks present in
    that many distinct genomes; coverage and NG50 are against the genome's size from its .fai, N50 against the genome's own total
    block length; the two counts and NG50 / N50 are truncated to integers AFTER the averaging.  sizes: {genome name: bases} of the
    genomes instead of .fai files (a run that has them at hand)."""
    n_genomes = len(sizes) if sizes is not None else len(fai_paths)
    sizes = dict(sizes) if sizes is not None else genome_sizes(fai_paths)
    lengths = {}            # genome -> [(length, block id)] in file order
    members = {}            # block id -> genomes that have it
    for r in read_blocks(tsv_path):
        lengths.setdefault(r.genome, []).append((r.end - r.start, r.block_id))
        members.setdefault(r.block_id, set()).add(r.genome)
    for name in lengths:
        if name not in sizes:
            raise ValueError(f"{tsv_path}: no size for genome {name} (have {sorted(sizes)})")
    in_all = {b for b, gs in members.items() if len(gs) >= n_genomes}
    every = {g: [v for v, _ in rows] for g, rows in lengths.items()}
    shared = {g: [v for v, b in rows if b in in_all] for g, rows in lengths.items()}

    def avg(per_genome):
        return sum(per_genome(g) for g in every) / n_genomes

    smallest = min(sizes, key=lambda g: sizes[g])         # (the first of several of one size, in the order of the .fai files)
    out = {
        "Number_blocks": int(avg(lambda g: len(every[g]))),
        "Number_blocks_all_asm": int(avg(lambda g: len(shared[g]))),
        "Average_coverage": avg(lambda g: sum(every[g]) / sizes[g] * 100),
        "Average_coverage_all_asm": avg(lambda g: sum(shared[g]) / sizes[g] * 100),
        "Coverage_min_genome_size": sum(every[smallest]) / sizes[smallest] * 100,
        "Average_length": avg(lambda g: sum(every[g]) / len(every[g])),
        "Median_length": avg(lambda g: _median(every[g])),
        "Total_length": avg(lambda g: sum(every[g])),
        "NG50_length": int(avg(lambda g: _n50(every[g], sizes[g]))),
        "N50_length": int(avg(lambda g: _n50(every[g], sum(every[g])))),
    }
    return out


def stats_table(stats):
    "the header line and the statistics line, as the reference prints them"
    return "\t".join(STATS_COLUMNS) + "\n" + "\t".join(str(stats[c]) for c in STATS_COLUMNS) + "\n"


def _block_order(rows):
    "block ids ascending (numerically where they are numbers), each with the indices of its lines in file order"
    by_id = {}
    for i, r in enumerate(rows):
        by_id.setdefault(r.block_id, []).append(i)

    def key(b):
        return (0, int(b), "") if b.lstrip("-").isdigit() else (1, 0, b)
    return [(b, by_id[b]) for b in sorted(by_id, key=key)]


def block_divergence(ctx, genomes_by_name, blocks, k=K_DEFAULT, s=S_DEFAULT):
    """Per block and unordered pair of its genomes the Mash distance of the two intervals.  genomes_by_name: the name in column 2 ->
    resident device.Genome, or a callable that returns one (it is then freed after its sweep: one genome resident at a time).
    blocks: read_blocks' rows.  Returns dicts keyed by DIVERGENCE_COLUMNS: block ids ascending, pairs in the order of the block's
    lines.  One nts_minhash_intervals call per genome, one nts_minhash_pairs call for all pairs; the strand is ignored (the hash is
    canonical)."""
    import numpy as np
    from .divergence import distance_of_counts
    k, s = int(k), int(s)
    n = len(blocks)
    sketches = np.zeros((n, s), dtype=np.uint64)
    counts = np.zeros(n, dtype=np.uint32)
    kmers = np.zeros(n, dtype=np.uint64)
    lines_of = {}
    for i, r in enumerate(blocks):
        lines_of.setdefault(r.genome, []).append(i)
    for name, lines in lines_of.items():
        if name not in genomes_by_name:
            raise ValueError(f"block table names genome {name}, which is not among {sorted(genomes_by_name)}")
        g = genomes_by_name[name]
        loaded = callable(g)
        if loaded:
            g = g()
        try:
            rec_of = {c: j for j, c in enumerate(g.names)}
            iv = np.zeros((len(lines), 3), dtype=np.uint64)
            for q, i in enumerate(lines):
                r = blocks[i]
                if r.contig not in rec_of:
                    raise ValueError(f"block {r.block_id}: genome {name} has no record {r.contig}")
                iv[q] = (rec_of[r.contig], max(r.start, 0), max(r.end, 0))
            sk, cnt, nk = g.minhash_intervals(iv, k, s)
        finally:
            if loaded:
                g.free()
        sketches[lines], counts[lines], kmers[lines] = sk, cnt, nk
    pair_a, pair_b, ids = [], [], []
    for b, lines in _block_order(blocks):
        for x in range(len(lines)):
            for y in range(x + 1, len(lines)):
                pair_a.append(lines[x])
                pair_b.append(lines[y])
                ids.append(b)
    shared, size = ctx.minhash_pairs(sketches, counts, pair_a, pair_b) if ids else ((), ())
    out = []
    for b, a_, b_, sh, sz in zip(ids, pair_a, pair_b, shared, size):
        out.append({"block_id": b, "genome_a": blocks[a_].genome, "genome_b": blocks[b_].genome, "distance": distance_of_counts(sh, sz, k),
                    "shared_hashes": int(sh), "sketch_size": int(sz), "kmers_a": int(kmers[a_]), "kmers_b": int(kmers[b_])})
    return out


def divergence_table(rows, k, s):
    "TSV with a header, one line per block and pair, then `# k K, sketch S`"
    lines = ["\t".join(DIVERGENCE_COLUMNS)]
    for r in rows:
        lines.append(f"{r['block_id']}\t{r['genome_a']}\t{r['genome_b']}\t{r['distance']:.6g}\t{r['shared_hashes']}\t{r['sketch_size']}\t"
                     f"{r['kmers_a']}\t{r['kmers_b']}")
    lines.append(f"# k {int(k)}, sketch {int(s)}")
    return "\n".join(lines) + "\n"


WIDE_NOT_WITH_VARIANTS = ("--identity-max-edits does not go with the block variants: the scripts of the wide stretches (more than 31 diagonals off the "
                          "main one) are not listed yet in block_variants.tsv -- --block-wide-variants (ntsynt_block_stats --wide-variants-out) writes a "
                          "file of its own that holds them")
WIDE_VARIANTS_NEED_E = ("the block wide variants list the stretches beyond the band and need --identity-max-edits E > 0 (2 * --identity-band + 1 .. 1023); "
                        "--block-variants (ntsynt_block_stats --variants-out) lists the edits of the band alone")


def check_identity_parameters(k, rate, band, max_len, max_edits=0):
    """the ranges of the parameters of the block identity; the message of the first that is out of range, or None.  max_edits: 0 = no wide
    pass, else 2 band + 1 .. 1023 (everything the narrow pass aligns has at most 2 band + 1 edits)"""
    if k < 1:
        return "--identity-k must be positive"
    if rate < 1:
        return "--identity-rate must be positive"
    if not 1 <= band <= 31:
        return "--identity-band must lie in 1..31"
    if not 1 <= max_len <= 65535:
        return "--identity-max-len must lie in 1..65535"
    if max_edits != 0 and not 2 * band + 1 <= max_edits <= 1023:
        return f"--identity-max-edits must be 0 (off) or lie in 2 * --identity-band + 1 = {2 * band + 1}..1023"
    return None


# one call's worth of pairs: the two resident genomes, A's intervals and per interval of A its mate's interval and flip, the segments and
# anchors nts_iv_anchor_segments found, and the pairs served as (line a, line b, index of a's interval)
_Round = namedtuple("_Round", ["name_a", "name_b", "g_a", "g_b", "iv_a", "iv_b", "flip", "segs", "anchors", "lines"])


def _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length, star=False):
    """The loop of block_identity and block_variants over pairs of genomes and rounds, as a generator of _Round.  Appends the pairs
    (line a, line b) in the order of the file's rows to `pairs` before the first round and fills length[line] = its clipped length as
    genomes become resident.  One nts_sample_intervals per genome over all its lines; per ordered pair of genomes one
    nts_iv_anchor_segments for every round of pairs in which no line of the first genome occurs twice; the consumer makes the edit
    calls on what a round holds before it asks for the next (the genomes of a round are resident until then).  star: only the STAR
    pairs (a block's first line, each of its other lines) are made -- a subset of the pairs, in their order."""
    import numpy as np
    from .device import NO_MATE
    lines_of, index_of = {}, {}
    for i, r in enumerate(blocks):
        index_of[i] = len(lines_of.setdefault(r.genome, []))
        lines_of[r.genome].append(i)
    for name in lines_of:
        if name not in genomes_by_name:
            raise ValueError(f"block table names genome {name}, which is not among {sorted(genomes_by_name)}")
    for _, lines in _block_order(blocks):                     # (line a, line b) in the order of the file's rows
        pairs += [(lines[x], lines[y]) for x in range(1 if star else len(lines)) for y in range(x + 1, len(lines))]
    rounds = {}                                               # (genome a, genome b) -> rounds of pairs, a line of a once per round
    for p in pairs:
        todo = rounds.setdefault((blocks[p[0]].genome, blocks[p[1]].genome), [])
        for rnd in todo:
            if p[0] not in rnd:
                rnd[p[0]] = p[1]
                break
        else:
            todo.append({p[0]: p[1]})
    last_use = {}
    for q, (ga, gb) in enumerate(rounds):
        last_use[ga] = last_use[gb] = q
    resident, loaded, intervals, records = {}, set(), {}, {}

    def genome(name):
        if name not in resident:
            g = genomes_by_name[name]
            if callable(g):
                g = g()
                loaded.add(name)
            resident[name] = g
            rec_of = {c: j for j, c in enumerate(g.names)}
            iv = np.zeros((len(lines_of[name]), 3), dtype=np.uint64)
            for q, i in enumerate(lines_of[name]):
                r = blocks[i]
                if r.contig not in rec_of:
                    raise ValueError(f"block {r.block_id}: genome {name} has no record {r.contig}")
                n = int(g.rec_len[rec_of[r.contig]])
                a, b = min(max(r.start, 0), n), min(max(r.end, 0), n)
                iv[q] = (rec_of[r.contig], a, max(a, b))
                length[i] = max(b - a, 0)
            intervals[name] = iv
            records[name] = g.sample_intervals(iv, k, rate)[0]
        return resident[name]
    try:
        for q, ((name_a, name_b), todo) in enumerate(rounds.items()):
            g_a, g_b = genome(name_a), genome(name_b)
            n_a = len(lines_of[name_a])
            for rnd in todo:
                mate = np.full(n_a, NO_MATE, dtype=np.uint32)
                len_b = np.zeros(n_a, dtype=np.uint32)
                flip = np.zeros(n_a, dtype=np.uint8)
                iv_b = np.zeros((n_a, 3), dtype=np.uint64)
                for la, lb in rnd.items():
                    i = index_of[la]
                    mate[i], len_b[i], flip[i] = index_of[lb], length[lb], blocks[la].strand != blocks[lb].strand
                    iv_b[i] = intervals[name_b][index_of[lb]]
                segs, anchors = ctx.iv_anchor_segments(records[name_a], records[name_b], mate, len_b, flip, k, band, max_len)
                yield _Round(name_a, name_b, g_a, g_b, intervals[name_a], iv_b, flip, segs, anchors, [(la, lb, index_of[la]) for la, lb in rnd.items()])
            for name in (name_a, name_b):
                if last_use[name] == q and name in loaded and name in resident:
                    resident.pop(name).free()
                    loaded.discard(name)
    finally:
        for name in loaded:
            if name in resident:
                resident[name].free()


def _identity_rows(blocks, pairs, length, found):
    "the dicts block_identity returns, from found[(line a, line b)] = (anchors, the interval's nts_iv_identity)"
    out = []
    for la, lb in pairs:
        anchors, s = found[(la, lb)]
        ra, rb = blocks[la], blocks[lb]
        out.append({"block_id": ra.block_id, "genome_a": ra.genome, "genome_b": rb.genome, "orientation": "+" if ra.strand == rb.strand else "-",
                    "length_a": length[la], "length_b": length[lb], "anchors": anchors, "segments": int(s["segments"]), "aligned": int(s["aligned"]),
                    "aligned_a": int(s["aligned_a"]), "aligned_b": int(s["aligned_b"]), "edits": int(s["edits"]), "backward": int(s["backward"]),
                    "long": int(s["too_long"]), "offband": int(s["offband"]), "invalid": int(s["invalid"]), "overband": int(s["overband"])})
    return out


def block_identity(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0):
    """Per block and unordered pair of its lines (a before b in file order) the exact edit distance between consecutive anchors.
    genomes_by_name: the name in column 2 -> resident device.Genome, or a callable that returns one: it is called once, and the genome
    is freed after the last pair that needs it (both genomes of a pair are resident at once).  blocks: read_blocks' rows.  Returns
    dicts of integers and names (identity_row formats one): block ids ascending, pairs in the order of the block's lines.  One
    nts_sample_intervals per genome over all its lines; per ordered pair of genomes one nts_iv_anchor_segments and one
    nts_edit_segments for every round of pairs in which no line of the first genome occurs twice.  max_edits = E > 0: behind each of
    them one nts_edit_wide on its per-segment results -- the stretches the band leaves out (offband with |dy - dx| <= E, overband) get
    their unrestricted distance where it is at most E, and the sums are those over the final results
    (docs/design/04_18_block_identity_wide.md)."""
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits))
    if message:
        raise ValueError(message)
    k, rate, band, max_len, max_edits = int(k), int(rate), int(band), int(max_len), int(max_edits)
    pairs, length, found = [], {}, {}
    for r in _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length):
        if max_edits > 0:
            _, dist = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, with_distances=True)
            per_iv, _ = ctx.edit_wide(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, dist)
        else:
            per_iv = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band)
        for la, lb, i in r.lines:
            found[(la, lb)] = (int(r.anchors[i]), per_iv[i])
    return _identity_rows(blocks, pairs, length, found)


def block_variants(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN):
    """block_identity and, from the same pass, the edits behind every pair's `edits`: returns (identity rows, variant rows).  Per
    round one nts_edit_segments with the per-segment distances and one nts_edit_script on them; the ops of a pair's segments become
    events (variant_events) in the coordinates of the two records.  Variant rows are dicts of VARIANT_COLUMNS (variant_row formats
    one): pairs in the order of the identity rows, events ascending by pos_a, then in script order."""
    import numpy as np
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len))
    if message:
        raise ValueError(message)
    k, rate, band, max_len = int(k), int(rate), int(band), int(max_len)
    pairs, length, found, events = [], {}, {}, {}
    for r in _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length):
        per_iv, dist = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, with_distances=True)
        ops, first = ctx.edit_script(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, dist)
        for la, lb, i in r.lines:
            found[(la, lb)] = (int(r.anchors[i]), per_iv[i])
            s0, s1 = (int(x) for x in np.searchsorted(r.segs["iv_a"], [i, i + 1]))          # (the segments come in iv_a order)
            mine = ops[int(first[s0]):int(first[s1])]
            if mine.size != int(per_iv[i]["edits"]):
                raise RuntimeError(f"block {blocks[la].block_id}: {mine.size} ops for {int(per_iv[i]['edits'])} edits")
            events[(la, lb)] = variant_events(mine, r.segs, int(r.iv_a[i][1]), int(r.iv_b[i][1]), length[lb], bool(r.flip[i]))
    rows = []
    for la, lb in pairs:
        ra, rb = blocks[la], blocks[lb]
        head = {"block_id": ra.block_id, "genome_a": ra.genome, "contig_a": ra.contig, "genome_b": rb.genome, "contig_b": rb.contig,
                "orientation": "+" if ra.strand == rb.strand else "-"}
        rows += [dict(head, **e) for e in events[(la, lb)]]
    return _identity_rows(blocks, pairs, length, found), rows


def block_wide_variants(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0):
    """block_identity with max_edits = E > 0 and, from the same pass, the edits behind every pair's `edits`, those of the stretches the
    band leaves out included: returns (identity rows under E, variant rows).  Per round nts_edit_segments with the per-segment
    distances, nts_edit_wide on them, nts_edit_script on the narrow distances and nts_edit_wide_script on the final ones; a segment's
    ops come from exactly one of the two script calls.  A pair's ops, in segment order, become events through variant_events, as
    block_variants makes them.  docs/design/04_19_block_wide_variants.md."""
    import numpy as np
    if int(max_edits) == 0:
        raise ValueError("block_wide_variants lists the stretches beyond the band and needs max_edits (--identity-max-edits) > 0; "
                         "block_variants (--block-variants) lists the edits of the band alone")
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits))
    if message:
        raise ValueError(message)
    k, rate, band, max_len, max_edits = int(k), int(rate), int(band), int(max_len), int(max_edits)
    pairs, length, found, events = [], {}, {}, {}
    for r in _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length):
        _, dist = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, with_distances=True)
        per_iv, final = ctx.edit_wide(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, dist)
        ops_n, first_n = ctx.edit_script(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, dist)
        ops_w, first_w = ctx.edit_wide_script(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, final)
        n_n, n_w = np.diff(first_n.astype(np.int64)), np.diff(first_w.astype(np.int64))
        if np.any((n_n > 0) & (n_w > 0)):
            raise RuntimeError("a segment has ops from both script calls")
        for la, lb, i in r.lines:
            found[(la, lb)] = (int(r.anchors[i]), per_iv[i])
            s0, s1 = (int(x) for x in np.searchsorted(r.segs["iv_a"], [i, i + 1]))          # (the segments come in iv_a order)
            parts = [ops_w[int(first_w[s]):int(first_w[s + 1])] if n_w[s] else ops_n[int(first_n[s]):int(first_n[s + 1])]
                     for s in range(s0, s1) if n_w[s] or n_n[s]]
            mine = np.concatenate(parts) if parts else ops_n[:0]
            if mine.size != int(per_iv[i]["edits"]):
                raise RuntimeError(f"block {blocks[la].block_id}: {mine.size} ops for {int(per_iv[i]['edits'])} edits")
            events[(la, lb)] = variant_events(mine, r.segs, int(r.iv_a[i][1]), int(r.iv_b[i][1]), length[lb], bool(r.flip[i]))
    rows = []
    for la, lb in pairs:
        ra, rb = blocks[la], blocks[lb]
        head = {"block_id": ra.block_id, "genome_a": ra.genome, "contig_a": ra.contig, "genome_b": rb.genome, "contig_b": rb.contig,
                "orientation": "+" if ra.strand == rb.strand else "-"}
        rows += [dict(head, **e) for e in events[(la, lb)]]
    return _identity_rows(blocks, pairs, length, found), rows


def check_ends_parameters(ends_max_len, ends_max_edits, ends_penalty):
    "the ranges of the parameters of the block ends; the message of the first that is out of range, or None"
    if not 1 <= ends_max_len <= 65535:
        return "--ends-max-len must lie in 1..65535"
    if not 1 <= ends_max_edits <= 1023:
        return "--ends-max-edits must lie in 1..1023"
    if not 3 <= ends_penalty <= 255:
        return "--ends-penalty must lie in 3..255 (below 3 an edit costs nothing)"
    return None


def ends_tasks(segs, final, iv_a, iv_b, flip, lines, rec_len_a, rec_len_b, ends_max_len):
    """The extension tasks of one round.  segs: the round's SEGMENT_DTYPE array in iv_a order, final: its final per-segment results;
    iv_a / iv_b: (rec, start, end) rows of the clipped intervals of A and of their mates, flip[i] = 1 for a pair of differing strands;
    lines: (line a, line b, index of a's interval); rec_len_*: the record lengths of the two genomes.  An interval with at least one
    segment whose result is a distance has a left end point (x, y_lo) of the first such segment and a right end point (x + dx,
    y_lo + dy) of the last one, oriented-frame offsets; from each a flank of at most ends_max_len bases runs outwards, past the
    interval, to the record's end at the furthest.  Returns (a TASK_DTYPE array, flanks): flanks[q] belongs to lines[q] and is None for
    a pair without an aligned segment, else dict(x_l, y_l, x_r, y_r, left, right) with the indices of its two tasks.  Pure."""
    import numpy as np
    from .device import EDIT_INVALID, EXTEND_A_BACKWARDS, EXTEND_B_BACKWARDS, EXTEND_B_COMPLEMENT, TASK_DTYPE
    cap = int(ends_max_len)
    tasks, flanks = [], []
    for _, _, i in lines:
        s0, s1 = (int(x) for x in np.searchsorted(segs["iv_a"], [i, i + 1]))                  # (the segments come in iv_a order)
        aligned = [s for s in range(s0, s1) if int(final[s]) < EDIT_INVALID]
        if not aligned:
            flanks.append(None)
            continue
        first, last = segs[aligned[0]], segs[aligned[-1]]
        x_l, y_l = int(first["x"]), int(first["y_lo"])
        x_r, y_r = int(last["x"]) + int(last["dx"]), int(last["y_lo"]) + int(last["dy"])
        rec_a, start_a = int(iv_a[i][0]), int(iv_a[i][1])
        rec_b, start_b, len_b = int(iv_b[i][0]), int(iv_b[i][1]), int(iv_b[i][2]) - int(iv_b[i][1])
        la, lb = int(rec_len_a[rec_a]), int(rec_len_b[rec_b])
        flipped = bool(flip[i])

        def task(pos_a, n, a_back, pos_b, m, b_back):
            "(a string of no base reads nothing: its position is put inside the record)"
            n, m = min(cap, n), min(cap, m)
            tasks.append((pos_a if n else 0, pos_b if m else 0, rec_a, rec_b, n, m,
                          (EXTEND_A_BACKWARDS if a_back else 0) | (EXTEND_B_BACKWARDS if b_back else 0) | (EXTEND_B_COMPLEMENT if flipped else 0), 0))
            return len(tasks) - 1
        if flipped:
            left = task(start_a + x_l - 1, start_a + x_l, True, start_b + len_b - y_l, lb - (start_b + len_b - y_l), False)
            right = task(start_a + x_r, la - (start_a + x_r), False, start_b + len_b - 1 - y_r, start_b + len_b - y_r, True)
        else:
            left = task(start_a + x_l - 1, start_a + x_l, True, start_b + y_l - 1, start_b + y_l, True)
            right = task(start_a + x_r, la - (start_a + x_r), False, start_b + y_r, lb - start_b - y_r, False)
        flanks.append({"x_l": x_l, "y_l": y_l, "x_r": x_r, "y_r": y_r, "left": left, "right": right})
    return np.array(tasks, dtype=TASK_DTYPE), flanks


def ends_stop(task, result, ends_max_len, ends_max_edits):
    """why a flank ends where it does.  The limit kind of a side: `invalid` when the string was cut at a base that is not A, C, G or T,
    else `max_len` when ends_max_len bases were asked for, else `record`.  The stop reason: A's limit kind when the extension used
    all of A, else B's when it used all of B, else `max_edits` when it spent them all, else `break`.  Pure."""
    def kind(valid, asked):
        return "invalid" if valid < asked else "max_len" if asked == int(ends_max_len) else "record"
    if int(result["ext_a"]) == int(result["valid_a"]):
        return kind(int(result["valid_a"]), int(task["n"]))
    if int(result["ext_b"]) == int(result["valid_b"]):
        return kind(int(result["valid_b"]), int(task["m"]))
    return "max_edits" if int(result["edits"]) == int(ends_max_edits) else "break"


def ends_row(ra, rb, iv_a, iv_b, flipped, flank, tasks, results, ends_max_len, ends_max_edits):
    """one pair's dict of ENDS_COLUMNS.  ra / rb: the two block lines, iv_a / iv_b: their clipped (rec, start, end); flank: the pair's
    entry of ends_tasks, tasks / results: that call's tasks and what nts_edit_extend made of them.  ext_* are half-open forward record
    coordinates: the interval from the left breakpoint to the right one; `.` throughout for a pair without flanks.  Pure."""
    start_a, end_a, start_b, end_b = int(iv_a[1]), int(iv_a[2]), int(iv_b[1]), int(iv_b[2])
    row = {"block_id": ra.block_id, "genome_a": ra.genome, "contig_a": ra.contig, "start_a": start_a, "end_a": end_a, "genome_b": rb.genome,
           "contig_b": rb.contig, "start_b": start_b, "end_b": end_b, "orientation": "-" if flipped else "+"}
    if flank is None:
        return dict(row, **{c: "." for c in ENDS_COLUMNS[10:]})
    left, right = results[flank["left"]], results[flank["right"]]
    for side, res, t in (("left", left, tasks[flank["left"]]), ("right", right, tasks[flank["right"]])):
        row[side + "_a"], row[side + "_b"], row[side + "_edits"] = int(res["ext_a"]), int(res["ext_b"]), int(res["edits"])
        row[side + "_stop"] = ends_stop(t, res, ends_max_len, ends_max_edits)
    row["ext_start_a"] = start_a + flank["x_l"] - row["left_a"]
    row["ext_end_a"] = start_a + flank["x_r"] + row["right_a"]
    if flipped:
        row["ext_end_b"] = end_b - flank["y_l"] + row["left_b"]
        row["ext_start_b"] = end_b - flank["y_r"] - row["right_b"]
    else:
        row["ext_start_b"] = start_b + flank["y_l"] - row["left_b"]
        row["ext_end_b"] = start_b + flank["y_r"] + row["right_b"]
    return row


def ends_table(rows, k, rate, band, max_len, max_edits, ends_max_len, ends_max_edits, ends_penalty):
    "TSV with a header, one line per block and pair of its lines, then the parameters of the identity pass and of the extension"
    lines = ["\t".join(ENDS_COLUMNS)] + ["\t".join(str(r[c]) for c in ENDS_COLUMNS) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}, max_edits {int(max_edits)}, ends_max_len {int(ends_max_len)}, "
                 f"ends_max_edits {int(ends_max_edits)}, ends_penalty {int(ends_penalty)}")
    return "\n".join(lines) + "\n"


def ends_events(ops, task, side):
    """The events of one flank.  ops: its OP_DTYPE entries in script order, p and q offsets in the task's two strings as
    nts_edit_extend reads them; task: its TASK_DTYPE entry (pos_a, pos_b, flags); side: `left` or `right`.  Runs are merged in the
    string frame as variant_events merges them: a maximal run of adjacent DEL ops with consecutive p and one q is one `del`, a maximal
    run of adjacent INS ops with one p and consecutive q one `ins`, every SUB an `snv`.  An event covers the string offsets
    [p0, p0 + La) of A and [q0, q0 + Lb) of B, either possibly empty; a string read forwards from pos holds them at the record
    positions [pos + p0, pos + p0 + L), one read backwards at [pos - p0 - L + 1, pos - p0 + 1).  Returns dicts of type, pos_a, pos_b
    (the starts of those forward intervals: for an empty one the boundary point, as variant_events has it), length = max(La, Lb),
    seq_a, seq_b -- the run's bases as read (B complemented for a pair of differing strands), reversed for the left flank so that both
    read along A's forward strand; `-` for no bases.  The right flank's events come in script order, the left flank's in reverse script
    order: both ascend along A's forward strand.  The script is canonical on the strings as read, which run OUTWARDS from the aligned
    core: inside a repeat an indel lies at the repeat's end nearest the core, so in forward coordinates a left flank's indel sits at the
    opposite end from a right flank's (no left-normalisation).  Pure."""
    sub, dele, ins = 1, 2, 3
    if side not in ("left", "right"):
        raise ValueError(f"not a flank: {side!r}")
    pos_a, pos_b, flags = int(task["pos_a"]), int(task["pos_b"]), int(task["flags"])
    a_back, b_back = bool(flags & 1), bool(flags & 2)         # (EXTEND_A_BACKWARDS, EXTEND_B_BACKWARDS)
    runs = []                                                 # [op, p0, q0, bases of A, bases of B]
    for _, p, q, op, base_a, base_b, _ in (ops.tolist() if hasattr(ops, "tolist") else ops):
        if op not in (sub, dele, ins) or (op != ins and base_a > 3) or (op != dele and base_b > 3):
            raise ValueError(f"not an edit op: {(p, q, op, base_a, base_b)}")
        last = runs[-1] if runs else None
        if last and last[0] == op == dele and p == last[1] + len(last[3]) and q == last[2]:
            last[3] += "ACGT"[base_a]
        elif last and last[0] == op == ins and p == last[1] and q == last[2] + len(last[4]):
            last[4] += "ACGT"[base_b]
        else:
            runs.append([op, p, q, "" if op == ins else "ACGT"[base_a], "" if op == dele else "ACGT"[base_b]])
    out = []
    for op, p0, q0, seq_a, seq_b in runs:
        if side == "left":
            seq_a, seq_b = seq_a[::-1], seq_b[::-1]
        out.append({"type": {sub: "snv", dele: "del", ins: "ins"}[op],
                    "pos_a": pos_a - p0 - len(seq_a) + 1 if a_back else pos_a + p0,
                    "pos_b": pos_b - q0 - len(seq_b) + 1 if b_back else pos_b + q0,
                    "length": max(len(seq_a), len(seq_b)), "seq_a": seq_a or "-", "seq_b": seq_b or "-"})
    return out[::-1] if side == "left" else out


def end_variant_row(r):
    "one line of the end variants table"
    return "\t".join(str(r[c]) for c in END_VARIANT_COLUMNS)


def end_variants_table(rows, k, rate, band, max_len, max_edits, ends_max_len, ends_max_edits, ends_penalty):
    "TSV of block_ends' variant rows: a header, one line per event of every flank, then the footer of ends_table"
    lines = ["\t".join(END_VARIANT_COLUMNS)] + [end_variant_row(r) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}, max_edits {int(max_edits)}, ends_max_len {int(ends_max_len)}, "
                 f"ends_max_edits {int(ends_max_edits)}, ends_penalty {int(ends_penalty)}")
    return "\n".join(lines) + "\n"


def block_ends(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0,
               ends_max_len=ENDS_MAX_LEN, ends_max_edits=ENDS_MAX_EDITS, ends_penalty=ENDS_PENALTY, with_variants=False):
    """Per block and pair of its lines the base-exact breakpoints: from the first and the last aligned stretch of block_identity (the same
    pairs, anchors, segments and final per-segment results for the same first five parameters) the alignment is extended outwards
    with a free end -- at most ends_max_len bases and ends_max_edits edits, each edit costing ends_penalty against 2 for a match --
    past the block's own interval.  Returns dicts of ENDS_COLUMNS in block_identity's order.  Per round block_identity's edit calls
    with the per-segment results and one nts_edit_extend over both flanks of all its pairs.  docs/design/04_20_block_ends.md.
    with_variants: returns (those rows, variant rows) -- dicts of END_VARIANT_COLUMNS, the events (ends_events) of every flank with at
    least one edit, pairs in the rows' order, the left flank before the right -- from one nts_edit_extend_script per round on that
    round's tasks and results; a flank whose number of ops is not its left_edits or right_edits raises RuntimeError.
    docs/design/04_21_block_end_variants.md."""
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        check_ends_parameters(int(ends_max_len), int(ends_max_edits), int(ends_penalty))
    if message:
        raise ValueError(message)
    k, rate, band, max_len, max_edits = int(k), int(rate), int(band), int(max_len), int(max_edits)
    cap, limit, penalty = int(ends_max_len), int(ends_max_edits), int(ends_penalty)
    pairs, length, found, events = [], {}, {}, {}
    for r in _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length):
        _, final = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, with_distances=True)
        if max_edits > 0:
            _, final = ctx.edit_wide(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, final)
        tasks, flanks = ends_tasks(r.segs, final, r.iv_a, r.iv_b, r.flip, r.lines, r.g_a.rec_len, r.g_b.rec_len, cap)
        results = ctx.edit_extend(r.g_a, r.g_b, tasks, penalty, limit)
        if with_variants:
            ops, first = ctx.edit_extend_script(r.g_a, r.g_b, tasks, results)
        for (la, lb, i), flank in zip(r.lines, flanks):
            found[(la, lb)] = ends_row(blocks[la], blocks[lb], r.iv_a[i], r.iv_b[i], bool(r.flip[i]), flank, tasks, results, cap, limit)
            if not with_variants:
                continue
            events[(la, lb)] = []
            for side in ("left", "right") if flank is not None else ():
                t = flank[side]
                mine = ops[int(first[t]):int(first[t + 1])]
                if mine.size != int(results[t]["edits"]):
                    raise RuntimeError(f"block {blocks[la].block_id}: {mine.size} ops for the {int(results[t]['edits'])} edits of a {side} flank")
                events[(la, lb)] += [dict(e, flank=side) for e in ends_events(mine, tasks[t], side)]
    rows = [found[p] for p in pairs]
    if not with_variants:
        return rows
    variant_rows = []
    for (la, lb), row in zip(pairs, rows):
        head = {"block_id": row["block_id"], "genome_a": row["genome_a"], "contig_a": row["contig_a"], "genome_b": row["genome_b"],
                "contig_b": row["contig_b"], "orientation": row["orientation"]}
        variant_rows += [dict(head, **e) for e in events[(la, lb)]]
    return rows, variant_rows


def alignment_pieces(segs, final, lines, flanks=None, results=None):
    """The chains of one round and the pieces nts_cigar_build stitches them from.  segs: the round's SEGMENT_DTYPE array in iv_a order,
    final: its final per-segment results; lines: (line a, line b, index of a's interval); flanks / results: what ends_tasks and
    nts_edit_extend made of the round, or None for chains without flanks.  A CHAIN is a maximal run of consecutive segments of one
    interval whose result is a distance (contiguous in x and y: a segment ends at the anchor the next one begins at); every other
    segment ends a chain and belongs to none.  One piece per segment of a chain, n = dx, m = dy; with flanks the left one is a reversed
    piece (n = ext_a, m = ext_b) in front of the pair's first chain and the right one a forward piece behind its last.  Returns
    (pieces, source, chains): a PIECE_DTYPE array in chain order; source[t] = the segment piece t stands for, or -1 - task for a flank;
    chains = dict of int64 arrays, one entry per chain in (iv_a, x) order -- line = index into `lines`, ch = the chain's number
    within its pair, x0, x1, y0, y1 = its oriented offsets, flanks included (they may leave the interval).  Pure."""
    import numpy as np
    from .device import CIG_REVERSED, EDIT_INVALID, PIECE_DTYPE
    n = len(segs)
    iv = segs["iv_a"].astype(np.int64)
    line_of = np.full(max([i for _, _, i in lines] + [int(iv.max()) if n else 0]) + 1, -1, dtype=np.int64)
    for q, (_, _, i) in enumerate(lines):
        line_of[i] = q
    aligned = (np.asarray(final, dtype=np.uint32) < EDIT_INVALID) & (line_of[iv] >= 0)
    follows = np.zeros(n, dtype=bool)                         # the segment in front is aligned and of the same interval
    follows[1:] = aligned[:-1] & (iv[1:] == iv[:-1])
    opens = aligned & ~follows
    chain_of = np.cumsum(opens) - 1                           # (where aligned)
    members = np.flatnonzero(aligned)
    heads = np.flatnonzero(opens)
    tails = members[np.append(chain_of[members][1:] != chain_of[members][:-1], True)] if members.size else members
    x, dx, y, dy = (segs[f].astype(np.int64) for f in ("x", "dx", "y_lo", "dy"))
    inner = members[follows[members]]
    if np.any(x[inner] != x[inner - 1] + dx[inner - 1]) or np.any(y[inner] != y[inner - 1] + dy[inner - 1]):
        raise ValueError("two consecutive aligned segments of an interval are not contiguous")
    line = line_of[iv[heads]]
    first_of_pair = np.append(True, line[1:] != line[:-1]) if heads.size else np.zeros(0, dtype=bool)
    last_of_pair = np.append(line[1:] != line[:-1], True) if heads.size else np.zeros(0, dtype=bool)
    number = np.arange(heads.size, dtype=np.int64)
    chains = {"line": line, "ch": number - np.maximum.accumulate(np.where(first_of_pair, number, 0)), "x0": x[heads].copy(), "x1": x[tails] + dx[tails],
              "y0": y[heads].copy(), "y1": y[tails] + dy[tails]}
    chain, size_n, size_m, flags, source, rank = chain_of[members], dx[members], dy[members], np.zeros(members.size, dtype=np.int64), members, \
        np.ones(members.size, dtype=np.int64)
    if flanks is not None:
        extra = []                                            # (chain, n, m, flags, source, rank: left 0 < segments 1 < right 2)
        for c in np.flatnonzero(first_of_pair | last_of_pair).tolist():
            flank = flanks[int(line[c])]
            if flank is None:
                raise ValueError("a pair with an aligned segment has no flanks")
            if first_of_pair[c]:
                if (flank["x_l"], flank["y_l"]) != (int(chains["x0"][c]), int(chains["y0"][c])):
                    raise ValueError("the left flank does not start at the pair's first chain")
                r = results[flank["left"]]
                extra.append((c, int(r["ext_a"]), int(r["ext_b"]), CIG_REVERSED, -1 - flank["left"], 0))
                chains["x0"][c] -= int(r["ext_a"])
                chains["y0"][c] -= int(r["ext_b"])
            if last_of_pair[c]:
                if (flank["x_r"], flank["y_r"]) != (int(chains["x1"][c]), int(chains["y1"][c])):
                    raise ValueError("the right flank does not start at the pair's last chain")
                r = results[flank["right"]]
                extra.append((c, int(r["ext_a"]), int(r["ext_b"]), 0, -1 - flank["right"], 2))
                chains["x1"][c] += int(r["ext_a"])
                chains["y1"][c] += int(r["ext_b"])
        if extra:
            more = np.array(extra, dtype=np.int64)
            chain, size_n, size_m, flags, source, rank = (np.concatenate([v, more[:, j]]) for j, v in enumerate((chain, size_n, size_m, flags, source, rank)))
    order = np.lexsort((source, rank, chain))                 # (segments of a chain ascend by index; a chain has at most one flank of a side)
    pieces = np.zeros(order.size, dtype=PIECE_DTYPE)
    pieces["chain"], pieces["n"], pieces["m"], pieces["flags"] = chain[order], size_n[order], size_m[order], flags[order]
    return pieces, source[order], chains


def alignment_ops(source, segment_scripts, flank_script=None):
    """The ops of alignment_pieces' pieces, re-based: segment_scripts = the (ops, first) pairs of the script calls over the round's
    segments -- a segment's ops are those of the LAST pair that holds any for it (nts_edit_script, then nts_edit_wide_script: no segment
    has ops from both); flank_script = (ops, first) of nts_edit_extend_script over the round's tasks.  Returns (ops, first) for
    nts_cigar_build: piece t's ops at ops[first[t]:first[t + 1]] with seg = t.  Pure; one gather, no loop over pieces or ops."""
    import numpy as np
    from .device import OP_DTYPE
    source = np.asarray(source, dtype=np.int64)
    start, count = np.zeros(source.size, dtype=np.int64), np.zeros(source.size, dtype=np.int64)
    parts, base = [], 0
    is_seg = source >= 0
    for ops, first in segment_scripts:
        first = np.asarray(first).astype(np.int64)
        have = np.diff(first)[source[is_seg]]
        take = np.flatnonzero(is_seg)[have > 0]
        start[take], count[take] = base + first[source[take]], have[have > 0]
        parts.append(ops)
        base += len(ops)
    if flank_script is not None and np.any(~is_seg):
        ops, first = flank_script
        first = np.asarray(first).astype(np.int64)
        task = -1 - source[~is_seg]
        start[~is_seg], count[~is_seg] = base + first[task], np.diff(first)[task]
        parts.append(ops)
    out_first = np.concatenate([[0], np.cumsum(count)]).astype(np.uint64)
    total = int(out_first[-1])
    if total == 0:
        return np.zeros(0, dtype=OP_DTYPE), out_first
    everything = np.concatenate(parts)
    index = np.repeat(start - out_first[:-1].astype(np.int64), count) + np.arange(total, dtype=np.int64)
    out = everything[index]
    out["seg"] = np.repeat(np.arange(source.size, dtype=np.uint32), count)
    return out, out_first


PAF_TAGS = ("NM:i:", "bi:i:", "tg:Z:", "qg:Z:", "ch:i:", "cg:Z:")


def cigar_texts(cigar, first, n_cig):
    """the cg:Z: strings of several chains at once: cigar = CIGAR entries len << 4 | code (I 1, D 2, = 7, X 8), chain c's at
    cigar[first[c]:first[c] + n_cig[c]].  Array operations over all entries (the numbers as fixed-width byte strings, the letters
    appended, the padding taken out of the whole buffer at once) and one slice per chain: no Python loop over entries.  Pure."""
    import numpy as np
    cigar = np.ascontiguousarray(cigar, dtype=np.uint64)
    first, n_cig = np.asarray(first).astype(np.int64), np.asarray(n_cig).astype(np.int64)
    if cigar.size == 0:
        return ["" for _ in range(first.size)]
    letters = np.full(16, b"?", dtype="S1")
    letters[[1, 2, 7, 8]] = [b"I", b"D", b"=", b"X"]
    tokens = np.char.add((cigar >> np.uint64(4)).astype("S20"), letters[(cigar & np.uint64(15)).astype(np.int64)])
    if np.any(tokens.view("S1").reshape(tokens.size, -1)[np.arange(tokens.size), np.char.str_len(tokens) - 1] == b"?"):
        raise ValueError("a CIGAR entry with a code that is not I, D, = or X")
    at = np.concatenate([[0], np.cumsum(np.char.str_len(tokens))])
    text = tokens.tobytes().replace(b"\0", b"").decode()
    return [text[at[a]:at[a + n]] for a, n in zip(first.tolist(), n_cig.tolist())]


def cigar_text(entries):
    "the cg:Z: string of one chain's CIGAR entries"
    return cigar_texts(entries, [0], [len(entries)])[0]


PAF_TAGS_CS = PAF_TAGS + ("cs:Z:",)


def alignment_spans(round, chains, flanks=None, results=None):
    """One nts_cig_span per chain of alignment_pieces, from what paf_row uses: round = the _Round (iv_a, iv_b, flip, lines), chains =
    alignment_pieces' dict, whose offsets already hold the flanks (flanks / results are not read again).  The target bases start at
    pos_a = start_a + x0 of a's record; the query bases at pos_b = start_b + y0 for `+`, and for `-` at start_b + L_b - y0 - 1, read
    downwards and complemented (CIG_B_BACKWARDS): the first base of the reverse complement of paf_row's query interval.  Array
    operations alone.  Pure."""
    import numpy as np
    from .device import CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    line = np.asarray(chains["line"], dtype=np.int64)
    spans = np.zeros(line.size, dtype=CIG_SPAN_DTYPE)
    if line.size == 0:
        return spans
    iv = np.array([i for _, _, i in round.lines], dtype=np.int64)[line]
    iv_a, iv_b = np.asarray(round.iv_a).astype(np.int64)[iv], np.asarray(round.iv_b).astype(np.int64)[iv]
    flipped = np.asarray(round.flip)[iv] != 0
    x0, y0 = np.asarray(chains["x0"], dtype=np.int64), np.asarray(chains["y0"], dtype=np.int64)
    pos_a = iv_a[:, 1] + x0
    pos_b = np.where(flipped, iv_b[:, 2] - y0 - 1, iv_b[:, 1] + y0)                        # (start_b + L_b = end_b)
    if np.any(pos_a < 0) or np.any(pos_b < -1):
        raise ValueError("a chain starts in front of its record")
    spans["pos_a"], spans["pos_b"] = pos_a.astype(np.uint64), np.maximum(pos_b, 0).astype(np.uint64)
    spans["rec_a"], spans["rec_b"], spans["flags"] = iv_a[:, 0], iv_b[:, 0], np.where(flipped, CIG_B_BACKWARDS, 0)
    return spans


def paf_row(ra, rb, rec_len_a, rec_len_b, iv_a, iv_b, flipped, ch, span, record, entries, cs=None):
    """one chain's PAF line (no newline).  ra / rb: the two block lines (a is the target, b the query), rec_len_*: the lengths of their
    records, iv_a / iv_b: their clipped (rec, start, end); span = (x0, x1, y0, y1), the chain's oriented offsets, flanks included;
    record: its nts_cig_chain fields (eq, x, ins, del), entries: its CIGAR entries, in a's forward order, or their cg:Z: text when
    the caller made the texts of many chains at once (cigar_texts); cs: the chain's cs:Z: text, appended behind cg:Z: (PAF_TAGS_CS),
    or None for the tags of PAF_TAGS.  Coordinates are 0-based and
    half-open on the forward strand of the records: for a `-` pair the query interval is mirrored inside b's interval.  Pure."""
    x0, x1, y0, y1 = (int(v) for v in span)
    start_a, start_b, len_b = int(iv_a[1]), int(iv_b[1]), int(iv_b[2]) - int(iv_b[1])
    eq, x, ins, dele = (int(record[f]) for f in ("eq", "x", "ins", "del"))
    q_from, q_to = (start_b + len_b - y1, start_b + len_b - y0) if flipped else (start_b + y0, start_b + y1)
    fields = [rb.contig, int(rec_len_b), q_from, q_to, "-" if flipped else "+", ra.contig, int(rec_len_a), start_a + x0, start_a + x1, eq, eq + x + ins + dele,
              255, f"NM:i:{x + ins + dele}", f"bi:i:{ra.block_id}", f"tg:Z:{ra.genome}", f"qg:Z:{rb.genome}", f"ch:i:{int(ch)}",
              "cg:Z:" + (entries if isinstance(entries, str) else cigar_text(entries))]
    if cs is not None:
        fields.append("cs:Z:" + cs)
    return "\t".join(str(f) for f in fields)


def paf_table(rows):
    "the PAF text of block_alignments' rows: one line per chain, no header and no footer (PAF has no comment syntax every reader accepts)"
    return "".join(r + "\n" for r in rows)


# what one round of the alignment pass produced: the _Round itself, the identity pass's per-interval sums, the flanks and their results (or
# None), the chains of alignment_pieces (one entry per chain: line, ch, x0, x1, y0, y1), nts_cigar_build's entries and records, and with
# cs nts_cigar_text's (cg, cg_first, cs, cs_first), and with maf nts_cigar_rows' (row_a, row_b, row_first) and the spans it was given
_AlignmentRound = namedtuple("_AlignmentRound", ["round", "per_iv", "flanks", "results", "chains", "cigar", "records", "texts", "rows"], defaults=(None, None))


def _alignment_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends, pairs, length, only=None, cs=False, maf=False, star=False):
    """The per-round body of block_alignments and block_lift over _identity_rounds, as a generator of _AlignmentRound: per round
    nts_edit_segments with the per-segment distances, for max_edits > 0 nts_edit_wide and both script calls, else nts_edit_script alone,
    with ends nts_edit_extend and nts_edit_extend_script, then ONE nts_cigar_build for all pairs of the round.  Per pair the NM of its
    chains less the flanks' edits must be the identity pass's `edits`, and the target and query bases less the flanks' must be aligned_a
    and aligned_b: RuntimeError otherwise.  only: a genome's name -- rounds in which it takes no part are passed over before any edit
    call.  cs: behind nts_cigar_build ONE nts_cigar_text per round over alignment_spans, its four arrays carried as `texts`; without it
    no call is added.  maf: behind nts_cigar_build ONE nts_cigar_rows per round over the same alignment_spans, its three arrays and the
    spans carried as `rows`; without it no call is added.  star: _identity_rounds' -- only the star pairs are made."""
    import numpy as np
    for r in _identity_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, pairs, length, star=star):
        if only is not None and only not in (r.name_a, r.name_b):
            continue
        per_iv, dist = ctx.edit_segments(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, with_distances=True)
        final = dist
        scripts = [ctx.edit_script(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, dist)]
        if max_edits > 0:
            per_iv, final = ctx.edit_wide(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, dist)
            scripts.append(ctx.edit_wide_script(r.g_a, r.g_b, r.iv_a, r.iv_b, r.segs, r.flip, band, max_edits, final))
            if np.any((np.diff(scripts[0][1].astype(np.int64)) > 0) & (np.diff(scripts[1][1].astype(np.int64)) > 0)):
                raise RuntimeError("a segment has ops from both script calls")
        tasks = flanks = results = flank_script = None
        if ends is not None:
            tasks, flanks = ends_tasks(r.segs, final, r.iv_a, r.iv_b, r.flip, r.lines, r.g_a.rec_len, r.g_b.rec_len, int(ends[0]))
            results = ctx.edit_extend(r.g_a, r.g_b, tasks, int(ends[2]), int(ends[1]))
            flank_script = ctx.edit_extend_script(r.g_a, r.g_b, tasks, results)
        pieces, source, chains = alignment_pieces(r.segs, final, r.lines, flanks, results)
        ops, first = alignment_ops(source, scripts, flank_script)
        cigar, records = ctx.cigar_build(pieces, ops, first, int(chains["line"].size))
        sums = np.zeros((3, len(r.lines)), dtype=np.int64)    # per pair: NM, target bases, query bases of its chains
        for row, values in enumerate((records["x"] + records["ins"] + records["del"], records["len_a"], records["len_b"])):
            np.add.at(sums[row], chains["line"], values.astype(np.int64))
        for q, (la, lb, i) in enumerate(r.lines):
            flank = flanks[q] if flanks is not None else None
            extra = [results[flank[side]] for side in ("left", "right")] if flank is not None else []
            nm, bases_a, bases_b = (int(v) for v in sums[:, q])
            if (nm - sum(int(e["edits"]) for e in extra), bases_a - sum(int(e["ext_a"]) for e in extra), bases_b - sum(int(e["ext_b"]) for e in extra)) != \
                    (int(per_iv[i]["edits"]), int(per_iv[i]["aligned_a"]), int(per_iv[i]["aligned_b"])):
                raise RuntimeError(f"block {blocks[la].block_id}: the chains of {blocks[la].genome} and {blocks[lb].genome} hold {nm} edits over {bases_a} and "
                                   f"{bases_b} bases, the identity pass {int(per_iv[i]['edits'])} over {int(per_iv[i]['aligned_a'])} and "
                                   f"{int(per_iv[i]['aligned_b'])} (flanks: {[tuple(int(v) for v in e) for e in extra]})")
        spans = alignment_spans(r, chains, flanks, results) if cs or maf else None
        texts = ctx.cigar_text(cigar, records, spans, r.g_a, r.g_b) if cs else None
        rows = ctx.cigar_rows(cigar, records, spans, r.g_a, r.g_b) + (spans,) if maf else None
        yield _AlignmentRound(r, per_iv, flanks, results, chains, cigar, records, texts, rows)


def _round_paf_rows(blocks, a, found):
    "found[(line a, line b)] = paf_row's lines of the pair's chains, ascending by x, for every pair of one round of the alignment pass"
    import numpy as np
    r, chains, records = a.round, a.chains, a.records
    cs_texts = None
    if a.texts is None:
        texts = cigar_texts(a.cigar, records["first"], records["n_cig"])
    else:                                                     # the device's texts: one decode per text, one slice per chain
        cg, cg_first, cs, cs_first = a.texts
        whole, at = cg.tobytes().decode(), cg_first.tolist()
        texts = [whole[at[c]:at[c + 1]] for c in range(len(at) - 1)]
        whole, at = cs.tobytes().decode(), cs_first.tolist()
        cs_texts = [whole[at[c]:at[c + 1]] for c in range(len(at) - 1)]
        if texts and texts[0] != cigar_texts(a.cigar, records["first"][:1], records["n_cig"][:1])[0]:
            raise RuntimeError(f"the device's cg text of the round's first chain is {texts[0][:60]!r}, the host's "
                               f"{cigar_texts(a.cigar, records['first'][:1], records['n_cig'][:1])[0][:60]!r}")
    line = chains["line"]
    by_line = np.argsort(line, kind="stable")                 # per pair its chains: one grouping of all chains by line
    cut = np.searchsorted(line[by_line], np.arange(len(r.lines) + 1))
    for q, (la, lb, i) in enumerate(r.lines):
        rec_len_a, rec_len_b = int(r.g_a.rec_len[int(r.iv_a[i][0])]), int(r.g_b.rec_len[int(r.iv_b[i][0])])
        found[(la, lb)] = [paf_row(blocks[la], blocks[lb], rec_len_a, rec_len_b, r.iv_a[i], r.iv_b[i], bool(r.flip[i]), chains["ch"][c],
                                   [chains[f][c] for f in ("x0", "x1", "y0", "y1")], records[c], texts[c], None if cs_texts is None else cs_texts[c])
                           for c in by_line[cut[q]:cut[q + 1]].tolist()]


def block_alignments(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None,
                     lift=None, lift_identity=None, cs=False, chain=False, maf=False):
    """One PAF record with a cg:Z: CIGAR per aligned chain of every block and pair of its lines (target = line a, query = line b): the
    anchors, segments and final per-segment results of block_identity for the same first five parameters, the canonical scripts of
    block_variants / block_wide_variants, and with ends = (ends_max_len, ends_max_edits, ends_penalty) the flanks of block_ends attached
    to each pair's first and last chain.  A pass of its own over the rounds (_alignment_rounds): per round nts_edit_segments with the
    per-segment distances, for max_edits > 0 nts_edit_wide and both script calls, else nts_edit_script alone, with ends nts_edit_extend
    and nts_edit_extend_script, then ONE nts_cigar_build for all pairs of the round.  Returns paf_row's lines: blocks and pairs in
    block_identity's order, a pair's chains ascending by x; a pair without an aligned segment has none.  Per pair the NM of its chains
    less the flanks' edits must be the identity pass's `edits`, and the target and query bases less the flanks' must be aligned_a and
    aligned_b: RuntimeError otherwise.  docs/design/04_22_block_alignments.md.  lift = (source, intervals): the same pass also lifts
    read_bed's intervals of the genome `source` (block_lift); returns (those lines, block_lift's rows).  lift_identity = (source,
    [intervals, ...]): the same pass also counts the alignment columns of every set of intervals (block_lift_identity; a set that IS
    the lift's dict is joined once for both); returns (those lines, block_lift's rows or None, [block_lift_identity's rows per set]).
    cs: every line also carries the cs:Z: tag (short form) behind cg:Z:, both texts made by ONE nts_cigar_text per round
    (docs/design/04_26_block_paf_cs.md); without it no call, launch or byte changes.  chain: the same pass also makes the liftover chains
    (block_chains: ONE nts_cigar_chain_blocks per round); chain_table's parts are appended to what is returned (a tuple then); without
    it no call, launch or byte changes.  maf: the same pass also makes the MAF blocks (block_mafs: ONE nts_cigar_rows per round;
    docs/design/04_29_block_maf.md); maf_table's parts are appended last to what is returned (a tuple then); without it no call, launch
    or byte changes."""
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        (check_ends_parameters(*(int(v) for v in ends)) if ends is not None else None)
    if message:
        raise ValueError(message)
    k, rate, band, max_len, max_edits = int(k), int(rate), int(band), int(max_len), int(max_edits)
    pairs, length, found, chains_of, mafs_of = [], {}, {}, {}, {}
    if lift_identity is not None:
        lifter = _lifter_of(genomes_by_name, blocks, lift, lift_identity)
    else:
        lifter = _Lifter(genomes_by_name, blocks, *lift) if lift is not None else None
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends, pairs, length, cs=bool(cs), maf=bool(maf)):
        _round_paf_rows(blocks, a, found)
        if lifter is not None:
            lifter.add_round(ctx, a, pairs)
        if chain:
            _round_chain_parts(ctx, blocks, a, chains_of)
        if maf:
            _round_maf_parts(blocks, a, mafs_of)
    rows = [row for p in pairs for row in found[p]]
    parts = ([chains_of[p] for p in pairs if chains_of.get(p) is not None],) if chain else ()
    if maf:
        parts += ([part for p in pairs for part in mafs_of[p]],)
    if lift_identity is not None:
        return (rows,) + lifter.results(genomes_by_name) + parts
    if lifter is not None:
        return (rows, lifter.rows(genomes_by_name)) + parts
    return (rows,) + parts if parts else rows


def chain_header(ra, rb, rec_len_a, rec_len_b, iv_a, iv_b, flipped, pair_record, base, chain_id):
    """the header line of one liftover chain (no newline): `chain score tName tSize + tStart tEnd qName qSize qStrand qStart qEnd id`.
    ra / rb, rec_len_*, iv_a / iv_b, flipped as for paf_row (a is the target, b the query); pair_record: the pair's nts_chain_pair
    fields (a0, a1, b0, b1, eq) in link offsets; base = (base_x, base_y) of chain_links: link offset + base = the oriented offset
    inside iv_a / iv_b.  score = eq.  The target is on its forward strand.  For a `-` pair the query coordinates lie on the query's
    REVERSE strand, as the format asks: paf_row's forward interval is [end_b - y1, end_b - y0), so qStart = qSize - (end_b - y0) and
    qEnd = qSize - (end_b - y1).  Pure."""
    x0, x1 = int(pair_record["a0"]) + int(base[0]), int(pair_record["a1"]) + int(base[0])
    y0, y1 = int(pair_record["b0"]) + int(base[1]), int(pair_record["b1"]) + int(base[1])
    start_a, start_b, end_b, q_size = int(iv_a[1]), int(iv_b[1]), int(iv_b[2]), int(rec_len_b)
    q_from, q_to = (q_size - end_b + y0, q_size - end_b + y1) if flipped else (start_b + y0, start_b + y1)
    return (f"chain {int(pair_record['eq'])} {ra.contig} {int(rec_len_a)} + {start_a + x0} {start_a + x1} {rb.contig} {q_size} {'-' if flipped else '+'} "
            f"{q_from} {q_to} {int(chain_id)}")


def chain_lines(blocks):
    "the data lines of one liftover chain from its CHAIN_BLOCK_DTYPE records, made on the host: the spot check of the device's text"
    rows = [(int(b["size"]), int(b["dt"]), int(b["dq"])) for b in blocks]
    return "".join(f"{s}\n" if j == len(rows) - 1 else f"{s}\t{t}\t{q}\n" for j, (s, t, q) in enumerate(rows))


def _round_chain_parts(ctx, blocks, a, found):
    """ONE nts_cigar_chain_blocks for a round of the alignment pass.  found[(line a, line b)] = chain_header's arguments without the id
    and the pair's slice of the device's text, or None for a pair without a liftover chain: one decode of the buffer and one slice per
    pair.  The lines of the round's first liftover chain are also made on the host and compared (RuntimeError)."""
    r = a.round
    links, pair_first, base_x, base_y = chain_links(a)
    pairs, chain_blocks, text, text_first = ctx.cigar_chain_blocks(a.cigar, a.records, links, pair_first.astype("uint64"))
    whole, at = text.tobytes().decode(), text_first.tolist()
    checked = False
    for q, (la, lb, i) in enumerate(r.lines):
        rec = pairs[q]
        if int(rec["n_blocks"]) == 0:
            found[(la, lb)] = None
            continue
        lines = whole[at[q]:at[q + 1]]
        if not checked:
            checked = True
            first = int(rec["first_block"])
            host = chain_lines(chain_blocks[first:first + int(rec["n_blocks"])])
            if lines != host:
                raise RuntimeError(f"the device's chain lines of the round's first liftover chain are {lines[:60]!r}, the host's {host[:60]!r}")
        rec_len_a, rec_len_b = int(r.g_a.rec_len[int(r.iv_a[i][0])]), int(r.g_b.rec_len[int(r.iv_b[i][0])])
        found[(la, lb)] = (blocks[la], blocks[lb], rec_len_a, rec_len_b, r.iv_a[i].copy(), r.iv_b[i].copy(), bool(r.flip[i]),
                           {f: int(rec[f]) for f in ("a0", "a1", "b0", "b1", "eq", "x", "n_blocks")}, (int(base_x[q]), int(base_y[q])), lines)


def chain_table(parts):
    """the UCSC chain file of block_chains' parts: per liftover chain chain_header's line, the pair's data lines as the device wrote
    them and a blank line; ids count from 1 in file order.  parts: per pair (chain_header's first nine arguments..., lines), in
    block_identity's pair order, pairs without a liftover chain left out"""
    return "".join(chain_header(*part[:9], n + 1) + "\n" + part[9] + "\n" for n, part in enumerate(parts))


def block_chains(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """One liftover chain per block and pair of its lines (target = line a, query = line b): the chains of block_alignments for the same
    parameters joined per pair, the stretch between two chains as a gap with bases on both sides (docs/design/04_28_block_chain.md).  A
    pass of its own over the rounds (_alignment_rounds) with ONE nts_cigar_chain_blocks per round, which makes the blocks and their
    text on the device.  Returns chain_table's parts in block_identity's pair order."""
    return block_alignments(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends, chain=True)[1]


MAF_HEADER = "##maf version=1\n\n"


def maf_block(name_a, rec_len_a, tstart, len_a, name_b, rec_len_b, qstart, qend, minus, eq, row_a, row_b):
    """the four lines of one pairwise MAF block: `a score=<eq>`, the target's `s` line, the query's `s` line and a blank line.  name_* =
    `<genome>.<contig>` (a is the target, b the query, as in paf_row and chain_header); tstart, qstart, qend: paf_row's forward
    coordinates; len_a: the target bases of the rows; row_a / row_b: the aligned rows (str), gaps as `-`.  The target is on `+`.  The
    start of a `-` line counts on the reverse strand, as the format asks: start_b = rec_len_b - qend, chain_header's convention.
    Fields are separated by one blank, without padding.  Pure."""
    start_b = int(rec_len_b) - int(qend) if minus else int(qstart)
    return (f"a score={int(eq)}\n"
            f"s {name_a} {int(tstart)} {int(len_a)} + {int(rec_len_a)} {row_a}\n"
            f"s {name_b} {start_b} {int(qend) - int(qstart)} {'-' if minus else '+'} {int(rec_len_b)} {row_b}\n\n")


def maf_table(parts):
    """the MAF text of block_mafs' parts: `##maf version=1`, a blank line, then maf_block's lines per chain in PAF order (blocks and pairs
    as in block_identity.tsv, a pair's chains ascending by x).  parts: per chain maf_block's arguments with `x` behind eq: (name_a,
    rec_len_a, tstart, len_a, name_b, rec_len_b, qstart, qend, minus, eq, x, row_a, row_b).  A chain with eq + x == 0 has no aligned base
    pair and gets no block: common readers refuse a block that is all gaps on one side."""
    return MAF_HEADER + "".join(maf_block(*part[:10], *part[11:]) for part in parts if int(part[9]) + int(part[10]) > 0)


_MAF_COMPLEMENT = None


def maf_rows_host(entries, target, query_as_read):
    """the two rows of one chain made on the host, as uint8 arrays: entries = its CIGAR entries, target / query_as_read = upper-case ASCII
    uint8 arrays of the bases the entries consume (the query already reverse-complemented for a `-` pair).  What is not ACGT shows as N.
    Array operations alone: one repeat over the entries and one scatter per row.  Pure: the spot check of nts_cigar_rows."""
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    kind = np.repeat((entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64))
    letters = np.full(256, ord("N"), dtype=np.uint8)
    letters[[ord(c) for c in "ACGT"]] = [ord(c) for c in "ACGT"]
    rows = []
    for seq, gap in ((target, 1), (query_as_read, 2)):       # I has no target base, D no query base
        row = np.full(kind.size, ord("-"), dtype=np.uint8)
        held = kind != gap
        if int(held.sum()) != len(seq):
            raise ValueError("the entries do not consume the bases given")
        row[held] = letters[np.asarray(seq, dtype=np.uint8)]
        rows.append(row)
    return rows[0], rows[1]


def _maf_revcomp(seq):
    import numpy as np
    global _MAF_COMPLEMENT
    if _MAF_COMPLEMENT is None:
        table = np.full(256, ord("N"), dtype=np.uint8)
        table[[ord(c) for c in "ACGT"]] = [ord(c) for c in "TGCA"]
        _MAF_COMPLEMENT = table
    return _MAF_COMPLEMENT[np.asarray(seq, dtype=np.uint8)[::-1]]


def _genome_bases(genome, rec, start, length):
    "upper-case ASCII of bases [start, start + length) of one record: from the genome's host copy where it has one, else one device read of that span"
    import numpy as np
    at = int(genome.rec_off[int(rec)]) + int(start)
    host = getattr(genome, "host_seq", None)
    if host is not None:
        return np.char.upper(np.asarray(host[at:at + int(length)]).view("S1")).view(np.uint8)
    return genome.download(at, int(length))


def _round_maf_parts(blocks, a, found):
    """found[(line a, line b)] = maf_table's parts of the pair's chains, ascending by x, for every pair of one round of the alignment pass
    made with maf: one decode per row buffer and one slice per chain.  The rows of the round's first chain with an aligned base pair are
    also made on the host (maf_rows_host over the genomes' bases) and compared (RuntimeError)."""
    import numpy as np
    r, chains, records = a.round, a.chains, a.records
    row_a, row_b, row_first, spans = a.rows
    whole_a, whole_b, at = row_a.tobytes().decode(), row_b.tobytes().decode(), row_first.tolist()
    line = chains["line"]
    by_line = np.argsort(line, kind="stable")                 # per pair its chains: one grouping of all chains by line
    cut = np.searchsorted(line[by_line], np.arange(len(r.lines) + 1))
    checked = False
    for q, (la, lb, i) in enumerate(r.lines):
        ra, rb, iv_a, iv_b, flipped = blocks[la], blocks[lb], r.iv_a[i], r.iv_b[i], bool(r.flip[i])
        rec_len_a, rec_len_b = int(r.g_a.rec_len[int(iv_a[0])]), int(r.g_b.rec_len[int(iv_b[0])])
        start_a, start_b, len_b = int(iv_a[1]), int(iv_b[1]), int(iv_b[2]) - int(iv_b[1])
        parts = []
        for c in by_line[cut[q]:cut[q + 1]].tolist():
            x0, y0, y1 = int(chains["x0"][c]), int(chains["y0"][c]), int(chains["y1"][c])
            q_from, q_to = (start_b + len_b - y1, start_b + len_b - y0) if flipped else (start_b + y0, start_b + y1)   # (paf_row's)
            rec = records[c]
            eq, x = int(rec["eq"]), int(rec["x"])
            mine_a, mine_b = whole_a[at[c]:at[c + 1]], whole_b[at[c]:at[c + 1]]
            if not checked and eq + x > 0:
                checked = True
                target = _genome_bases(r.g_a, iv_a[0], start_a + x0, int(rec["len_a"]))
                query = _genome_bases(r.g_b, iv_b[0], q_from, q_to - q_from)
                first = int(rec["first"])
                host_a, host_b = maf_rows_host(a.cigar[first:first + int(rec["n_cig"])], target, _maf_revcomp(query) if flipped else query)
                if (mine_a, mine_b) != (host_a.tobytes().decode(), host_b.tobytes().decode()):
                    raise RuntimeError(f"the device's MAF rows of the round's first block are {mine_a[:60]!r} and {mine_b[:60]!r}, the host's "
                                       f"{host_a[:60].tobytes().decode()!r} and {host_b[:60].tobytes().decode()!r}")
            parts.append((f"{ra.genome}.{ra.contig}", rec_len_a, start_a + x0, int(rec["len_a"]), f"{rb.genome}.{rb.contig}", rec_len_b, q_from, q_to, flipped,
                          eq, x, mine_a, mine_b))
        found[(la, lb)] = parts


def block_mafs(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """One pairwise MAF block per aligned chain of every block and pair of its lines (target = line a, query = line b): the chains of
    block_alignments for the same parameters with their aligned rows (docs/design/04_29_block_maf.md).  A pass of its own over the rounds
    (_alignment_rounds) with ONE nts_cigar_rows per round, which makes both rows of every chain on the device.  Returns maf_table's parts
    in PAF order."""
    return block_alignments(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends, maf=True)[1]

# ---- block multi-MAF: one reference-anchored block per synteny block (docs/design/04_30_block_maf_multi.md) ----

def chain_cores(cigar, records, spans):
    """The CORE of every chain: the chain without its leading and trailing I and D entries, from the first = or X entry to the last.
    cigar, records, spans as nts_cigar_build and alignment_spans give them.  Returns (first, n_cig, len_a, len_b, pos_a, pos_b), int64
    arrays per chain: where the core's entries lie in `cigar` and its span; n_cig = 0 for a chain without = or X, which takes no part.
    Array operations over the entries alone.  Pure."""
    import numpy as np
    from .device import CIG_B_BACKWARDS
    cigar = np.ascontiguousarray(cigar, dtype=np.uint64)
    first, n_cig = records["first"].astype(np.int64), records["n_cig"].astype(np.int64)
    code, size = (cigar & np.uint64(15)).astype(np.int64), (cigar >> np.uint64(4)).astype(np.int64)
    both = (code == 7) | (code == 8)
    sum_a = np.concatenate(([0], np.cumsum(np.where(both | (code == 2), size, 0))))
    sum_b = np.concatenate(([0], np.cumsum(np.where(both | (code == 1), size, 0))))
    chain_of = np.repeat(np.arange(first.size), n_cig)       # (the chains tile the entries)
    at = np.flatnonzero(both)
    lo, hi = np.full(first.size, cigar.size, dtype=np.int64), np.full(first.size, -1, dtype=np.int64)
    np.minimum.at(lo, chain_of[at], at)
    np.maximum.at(hi, chain_of[at], at)
    held = hi >= 0
    lo, hi = np.where(held, lo, first), np.where(held, hi + 1, first)
    cut_a, cut_b = sum_a[lo] - sum_a[first], sum_b[lo] - sum_b[first]
    back = (spans["flags"].astype(np.int64) & CIG_B_BACKWARDS) != 0
    pos_b = spans["pos_b"].astype(np.int64)
    return (lo, hi - lo, sum_a[hi] - sum_a[lo], sum_b[hi] - sum_b[lo], spans["pos_a"].astype(np.int64) + cut_a, np.where(back, pos_b - cut_b, pos_b + cut_b))


def multi_maf_col0(r0, site_pos, site_w, p):
    "col0(p) of a group that begins at reference base r0: p - r0 + the widths of its sites in front of slot p.  p: an int or an array.  Pure."
    import numpy as np
    before = np.concatenate(([0], np.cumsum(np.asarray(site_w, dtype=np.int64))))
    return np.asarray(p, dtype=np.int64) - int(r0) + before[np.searchsorted(np.asarray(site_pos, dtype=np.int64), p, side="left")]


def multi_maf_parts(ref_name, ref_len, chains, site_pos, site_w):
    """The sub-blocks of one group.  chains: per core chain, in (row, t0) order, (row, t0, t1, name, src_size, minus, start, row_a,
    row_b): row >= 1, [t0, t1) its reference bases, name = `<genome>.<contig>`, start = where its bases begin on the strand its `s` line
    counts on, row_a / row_b = its padded rows (str), col0(t1) - col0(t0) columns.  site_pos / site_w: the group's sites.  The cut
    points are the sorted distinct t0 and t1; per consecutive pair [c, c') the covering chains (at most one per row: ValueError) give the
    reference row -- row A of any of them, two are compared: RuntimeError -- and a row each; a row of `-` alone is left out and a
    sub-block with fewer than two rows is not written.  Returns per sub-block a list of `s` line fields (name, start, size, strand,
    src_size, row), the reference first.  One slice per chain and sub-block, sizes from str.count: no loop over columns.  Pure."""
    import numpy as np
    if not chains:
        return []
    r0 = min(int(ch[1]) for ch in chains)
    cuts = sorted({int(t) for ch in chains for t in ch[1:3]})
    cols = multi_maf_col0(r0, site_pos, site_w, np.array(cuts, dtype=np.int64)).tolist()
    base = multi_maf_col0(r0, site_pos, site_w, np.array([int(ch[1]) for ch in chains], dtype=np.int64)).tolist()
    for prev, ch in zip(chains[:-1], chains[1:]):
        if prev[0] == ch[0] and int(ch[1]) < int(prev[2]):
            raise ValueError(f"two chains of row {ch[0]} overlap in the reference at base {int(ch[1])}")
    seen = [int(ch[6]) for ch in chains]                     # the running base count of every chain's row
    out = []
    for (c, c_next), (lo, hi) in zip(zip(cuts[:-1], cuts[1:]), zip(cols[:-1], cols[1:])):
        reference, lines, compared = None, [], False
        for j, ch in enumerate(chains):
            if not (int(ch[1]) <= c and c_next <= int(ch[2])):
                continue
            piece_a, piece_b = ch[7][lo - base[j]:hi - base[j]], ch[8][lo - base[j]:hi - base[j]]
            if reference is None:
                reference = piece_a
            elif not compared:
                compared = True
                if piece_a != reference:
                    raise RuntimeError(f"the chains that cover reference bases {c} .. {c_next} of {ref_name} disagree about the reference row")
            size = len(piece_b) - piece_b.count("-")
            if size:
                lines.append((ch[3], seen[j], size, "-" if ch[5] else "+", int(ch[4]), piece_b))
            seen[j] += size
        if lines:
            out.append([(ref_name, c, len(reference) - reference.count("-"), "+", int(ref_len), reference)] + lines)
    return out


def multi_maf_table(parts):
    "the text of the multi-MAF file: MAF_HEADER, then per sub-block `a`, one `s` line per row and a blank line.  parts: multi_maf_parts' lists, in file order.  Pure."
    return MAF_HEADER + "".join("a\n" + "".join(f"s {n} {st} {sz} {sd} {src} {row}\n" for n, st, sz, sd, src, row in block) + "\n" for block in parts)


def padded_rows_host(entries, target, query_as_read):
    "maf_rows_host for padded entries: a column of code 6 is `-` in both rows and consumes nothing.  Pure: the spot check of block_multi_mafs."
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    kind = np.repeat((entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64))
    letters = np.full(256, ord("N"), dtype=np.uint8)
    letters[[ord(c) for c in "ACGT"]] = [ord(c) for c in "ACGT"]
    rows = []
    for seq, gap in ((target, 1), (query_as_read, 2)):
        row = np.full(kind.size, ord("-"), dtype=np.uint8)
        held = (kind != gap) & (kind != 6)
        if int(held.sum()) != len(seq):
            raise ValueError("the entries do not consume the bases given")
        row[held] = letters[np.asarray(seq, dtype=np.uint8)]
        rows.append(row)
    return rows[0].tobytes().decode(), rows[1].tobytes().decode()


def unpadded_host(entries):
    "padded entries without their P entries, the runs P split merged again: the core they were made from.  Array operations.  Pure."
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    kept = entries[(entries & np.uint64(15)) != np.uint64(6)]
    if kept.size == 0:
        return kept
    code = kept & np.uint64(15)
    head = np.concatenate(([True], code[1:] != code[:-1]))
    return (np.add.reduceat(kept >> np.uint64(4), np.flatnonzero(head)) << np.uint64(4)) | code[head]


def block_multi_mafs(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """One reference-anchored multiple alignment per synteny block (docs/design/04_30_block_maf_multi.md): the star pairs (first line,
    other line) of every block are aligned as block_alignments aligns them (_alignment_rounds with star), every chain is trimmed to its
    core, the cores ordered by (block, row, x) get their gap columns from ONE nts_cigar_pad, and per pair of genomes ONE
    nts_cigar_rows_padded makes the rows of that pair's padded chains, which multi_maf_parts cuts into sub-blocks.  Genomes given as
    callables are loaded a second time for the rows, each query one at a time beside the reference's genome.  The first group's padded
    entries are checked on the host (unpadded_host gives the cores back; every chain has col0(t1) - col0(t0) columns) and the rows of its
    first chain are made on the host and compared: RuntimeError.  Returns multi_maf_table's parts."""
    import numpy as np
    from .device import CHAIN_DTYPE, CIG_B_BACKWARDS, CIG_SPAN_DTYPE
    n_groups, held, entries, records, at = _star_cores(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends)
    if not held:
        return []
    padded, pad_first, site_first, site_pos, site_w = ctx.cigar_pad(entries, records, at, n_groups)
    pad_first, site_first = pad_first.astype(np.int64), site_first.astype(np.int64)
    group_of = at["group"].astype(np.int64)
    # the rows: per pair of genomes ONE call over that pair's padded chains
    rows = [None] * len(held)
    by_pair = {}
    for j, h in enumerate(held):
        by_pair.setdefault((blocks[h[10]].genome, blocks[h[11]].genome), []).append(j)
    loaded = {}

    def genome(name):
        if name not in loaded:
            g = genomes_by_name[name]
            loaded[name] = (g(), True) if callable(g) else (g, False)
        return loaded[name][0]

    def release(name):
        g, mine = loaded.pop(name)
        if mine:
            g.free()
    try:
        for (name_a, name_b), members in by_pair.items():
            for name in [n for n in loaded if n not in (name_a, name_b)]:
                release(name)
            sub = np.zeros(len(members), dtype=CHAIN_DTYPE)
            sub["n_cig"] = (pad_first[1:] - pad_first[:-1])[members]
            sub["first"] = np.concatenate(([0], np.cumsum(sub["n_cig"][:-1].astype(np.int64))))
            sub["len_a"], sub["len_b"] = records["len_a"][members], records["len_b"][members]
            spans = np.zeros(len(members), dtype=CIG_SPAN_DTYPE)
            spans["pos_a"], spans["pos_b"] = [held[j][2] for j in members], [held[j][6] for j in members]
            spans["rec_a"], spans["rec_b"], spans["flags"] = [held[j][7] for j in members], [held[j][8] for j in members], [held[j][9] for j in members]
            mine = np.concatenate([padded[pad_first[j]:pad_first[j + 1]] for j in members])
            g_a, g_b = genome(name_a), genome(name_b)
            row_a, row_b, row_first = ctx.cigar_rows(mine, sub, spans, g_a, g_b, padded=True)
            whole_a, whole_b, cut = row_a.tobytes().decode(), row_b.tobytes().decode(), row_first.tolist()
            for q, j in enumerate(members):
                rows[j] = (whole_a[cut[q]:cut[q + 1]], whole_b[cut[q]:cut[q + 1]])
            if members[0] == 0:                              # the spot check: the first group's entries, the first chain's rows
                for j in np.flatnonzero(group_of == group_of[0]).tolist():
                    h = held[j]
                    sites = slice(site_first[h[0]], site_first[h[0] + 1])
                    r0 = min(held[i][2] for i in np.flatnonzero(group_of == group_of[0]).tolist())
                    want = int(multi_maf_col0(r0, site_pos[sites], site_w[sites], h[2] + h[4]) - multi_maf_col0(r0, site_pos[sites], site_w[sites], h[2]))
                    mine_j = padded[pad_first[j]:pad_first[j + 1]]
                    if not np.array_equal(unpadded_host(mine_j), unpadded_host(h[3])) or int((mine_j >> np.uint64(4)).sum()) != want:
                        raise RuntimeError(f"block {blocks[h[10]].block_id}: the padded CIGAR of a chain of {blocks[h[11]].genome} is not its core in {want} columns")
                h = held[0]
                back = bool(h[9] & CIG_B_BACKWARDS)
                target = _genome_bases(g_a, h[7], h[2], h[4])
                query = _genome_bases(g_b, h[8], h[6] - h[5] + 1 if back else h[6], h[5])
                host = padded_rows_host(padded[pad_first[0]:pad_first[1]], target, _maf_revcomp(query) if back else query)
                if host != rows[0]:
                    raise RuntimeError(f"the device's padded rows of the first chain are {rows[0][0][:60]!r} and {rows[0][1][:60]!r}, the host's "
                                       f"{host[0][:60]!r} and {host[1][:60]!r}")
    finally:
        for name in list(loaded):
            release(name)
    parts = []
    cut = np.searchsorted(group_of, np.arange(n_groups + 1))
    for g in range(n_groups):
        members = range(int(cut[g]), int(cut[g + 1]))
        if not len(members):
            continue
        ref = blocks[held[members[0]][10]]
        chains = []
        for j in members:
            h = held[j]
            back, rb = bool(h[9] & CIG_B_BACKWARDS), blocks[h[11]]
            start = h[13] - h[6] - 1 if back else h[6]        # (a `-` row counts on the reverse strand: rec_len_b - q_to, q_to = pos_b + 1)
            chains.append((h[1], h[2], h[2] + h[4], f"{rb.genome}.{rb.contig}", h[13], back, start, rows[j][0], rows[j][1]))
        sites = slice(site_first[g], site_first[g + 1])
        parts += multi_maf_parts(f"{ref.genome}.{ref.contig}", held[members[0]][12], chains, site_pos[sites], site_w[sites])
    return parts


def _star_cores(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends):
    """The core chains of every block's star pairs (first line, other line), as block_multi_mafs and block_conservation read them: the
    pairs are aligned as block_alignments aligns them (_alignment_rounds with star), every chain is trimmed to its core (chain_cores) and
    the cores are ordered by (block, row, x).  Two chains of one row that overlap in the reference raise ValueError.  Returns (n_groups,
    held, entries, records, at): the number of blocks (a group each, in block_identity.tsv's order); per core chain (group, row, pos_a,
    its entries, len_a, len_b, pos_b, rec_a, rec_b, span flags, line a, line b, rec_len_a, rec_len_b); and the chains' entries one behind
    the other with their CHAIN_DTYPE records and CIG_PAD_AT_DTYPE {group, t0}: what nts_cigar_pad and nts_cigar_depth take (None where no
    chain is held)."""
    import numpy as np
    from .device import CHAIN_DTYPE, CIG_PAD_AT_DTYPE
    pairs, length = [], {}
    order = {lines[0]: (g, lines) for g, (_, lines) in enumerate(_block_order(blocks))}        # first line -> (group, the block's lines)
    held = []                                                # per core chain: (group, row, pos_a, its entries, len_a, len_b, span fields, names ...)
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends, pairs, length, star=True):
        r, records = a.round, a.records
        spans = alignment_spans(r, a.chains, a.flanks, a.results)
        first, n_cig, len_a, len_b, pos_a, pos_b = chain_cores(a.cigar, records, spans)
        pair_of = [r.lines[q] for q in np.asarray(a.chains["line"]).tolist()]
        for c in np.flatnonzero(n_cig > 0).tolist():
            la, lb, _ = pair_of[c]
            group, lines = order[la]
            held.append((group, lines.index(lb), int(pos_a[c]), a.cigar[first[c]:first[c] + n_cig[c]], int(len_a[c]), int(len_b[c]), int(pos_b[c]),
                         int(spans["rec_a"][c]), int(spans["rec_b"][c]), int(spans["flags"][c]), la, lb, int(r.g_a.rec_len[int(spans["rec_a"][c])]),
                         int(r.g_b.rec_len[int(spans["rec_b"][c])])))
    held.sort(key=lambda h: h[:3])
    n_groups = len(order)
    if not held:
        return n_groups, held, None, None, None
    entries = np.concatenate([h[3] for h in held]).astype(np.uint64)
    records = np.zeros(len(held), dtype=CHAIN_DTYPE)
    records["n_cig"] = [h[3].size for h in held]
    records["first"] = np.concatenate(([0], np.cumsum(records["n_cig"][:-1].astype(np.int64))))
    records["len_a"], records["len_b"] = [h[4] for h in held], [h[5] for h in held]
    at = np.zeros(len(held), dtype=CIG_PAD_AT_DTYPE)
    at["group"], at["t0"] = [h[0] for h in held], [h[2] for h in held]
    for prev, h in zip(held[:-1], held[1:]):
        if prev[:2] == h[:2] and h[2] < prev[2] + prev[4]:
            raise ValueError(f"block {blocks[h[10]].block_id}: two chains of {blocks[h[11]].genome} overlap in the reference")
    return n_groups, held, entries, records, at

# ---- block conservation: per-base depth and identity over the star alignment (docs/design/04_31_block_conservation.md) ----

CONSERVATION_BED_COLUMNS = ("contig", "start", "end", "block_id", "genome", "rows", "aligned", "match", "mismatch", "gap")
CONSERVATION_COLUMNS = ("block_id", "genome", "contig", "start", "end", "rows", "covered", "core", "conserved", "by_aligned", "by_match")


def depth_segments_host(entries, records, at):
    """nts_cigar_depth's segments of ONE group on the host: a difference array per count over the group's reference extent, one
    cumulative sum each and a run-length encoding of the triples with aligned > 0.  entries, records, at: that group's chains (the
    records' `first` index `entries`).  Returns (start, end, aligned, match, gap), int64 arrays.  Array operations over entries and
    bases; the spot check of block_conservation and the baseline of scripts/block_conservation_measure.py.  Pure."""
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    code, size = (entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64)
    first, n_cig = records["first"].astype(np.int64), records["n_cig"].astype(np.int64)
    t0, len_a = at["t0"].astype(np.int64), records["len_a"].astype(np.int64)
    empty = np.zeros(0, dtype=np.int64)
    if t0.size == 0:
        return empty, empty, empty, empty, empty
    r0, r1 = int(t0.min()), int((t0 + len_a).max())
    uses = np.where(code == 1, 0, size)                      # the reference bases of every entry
    before = np.concatenate(([0], np.cumsum(uses)))
    chain_of = np.repeat(np.arange(first.size), n_cig)       # (the chains tile the entries)
    begin = t0[chain_of] - r0 + before[:-1] - before[first[chain_of]]
    counts = []
    for which in (code != 1, code == 7, code == 2):
        diff = np.zeros(r1 - r0 + 1, dtype=np.int64)
        np.add.at(diff, begin[which], 1)
        np.add.at(diff, (begin + uses)[which], -1)
        counts.append(np.cumsum(diff)[:-1])
    aligned, match, gap = counts
    if aligned.size == 0:
        return empty, empty, empty, empty, empty
    same = (aligned[1:] == aligned[:-1]) & (match[1:] == match[:-1]) & (gap[1:] == gap[:-1])
    head = np.flatnonzero(np.concatenate(([True], ~same)))
    tail = np.concatenate((head[1:], [aligned.size]))
    live = aligned[head] > 0
    head, tail = head[live], tail[live]
    return head + r0, tail + r0, aligned[head], match[head], gap[head]


def block_conservation(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """Per synteny block the reference bases that its genomes share and those that are identical in all of them
    (docs/design/04_31_block_conservation.md): the core chains of the star pairs (_star_cores, as block_multi_mafs collects them) go
    through ONE nts_cigar_depth, which gives every block's maximal runs of reference bases with one (aligned, match, gap).  The first
    group's segments are recomputed on the host (depth_segments_host) and compared: RuntimeError.  Returns (groups, segs, seg_first):
    per block, in block_identity.tsv's order, (block_id, genome, contig, start, end, rows) of its first line with rows = its lines - 1;
    the CIG_DEPTH_SEG_DTYPE segments and where each block's begin: what conservation_bed and conservation_table take."""
    import numpy as np
    from .device import CIG_DEPTH_SEG_DTYPE
    n_groups, held, entries, records, at = _star_cores(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends)
    groups = [(b, blocks[lines[0]].genome, blocks[lines[0]].contig, blocks[lines[0]].start, blocks[lines[0]].end, len(lines) - 1)
              for b, lines in _block_order(blocks)]
    if not held:
        return groups, np.zeros(0, dtype=CIG_DEPTH_SEG_DTYPE), np.zeros(n_groups + 1, dtype=np.uint64)
    segs, seg_first = ctx.cigar_depth(entries, records, at, n_groups)
    g0 = int(at["group"][0])                                  # the spot check: the first group that has chains
    mine = np.flatnonzero(at["group"] == g0)
    sub = records[mine].copy()
    sub["first"] -= records["first"][mine[0]]
    lo, hi = int(records["first"][mine[0]]), int(records["first"][mine[-1]] + records["n_cig"][mine[-1]])
    host = depth_segments_host(entries[lo:hi], sub, at[mine])
    got = segs[int(seg_first[g0]):int(seg_first[g0 + 1])]
    if any(not np.array_equal(got[f].astype(np.int64), h) for f, h in zip(("start", "end", "aligned", "match", "gap"), host)) or \
            np.any(got["group"] != g0):
        raise RuntimeError(f"block {groups[g0][0]}: the device's {got.size} conservation segments differ from the host's {host[0].size}")
    return groups, segs, seg_first


def conservation_summary(segs, seg_first, rows):
    """Per group the bases of its segments by depth.  segs, seg_first: nts_cigar_depth's; rows[g]: the rows of group g besides the
    reference (its lines - 1).  Returns a list of dicts: covered (aligned >= 1), core (aligned == rows), conserved (match == rows),
    by_aligned (bases per aligned = 1 .. rows, a list) and by_match (core bases per match = 0 .. rows, a list).  A segment with aligned
    > rows raises ValueError.  One np.add.at per histogram over all segments: no loop over segments or bases.  Pure."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    seg_first = np.asarray(seg_first, dtype=np.int64)
    n_groups = rows.size
    if seg_first.size != n_groups + 1:
        raise ValueError("conservation_summary: one entry of rows per group")
    group = np.repeat(np.arange(n_groups), seg_first[1:] - seg_first[:-1])
    size = segs["end"].astype(np.int64) - segs["start"].astype(np.int64)
    aligned, match = segs["aligned"].astype(np.int64), segs["match"].astype(np.int64)
    if np.any(aligned > rows[group]):
        raise ValueError("conservation_summary: a segment is covered by more chains than its group has rows")
    width = int(rows.max()) + 1 if n_groups else 1           # one histogram row per group: aligned or match 0 .. the most rows
    by_aligned, by_match = np.zeros((n_groups, width), dtype=np.int64), np.zeros((n_groups, width), dtype=np.int64)
    is_core = aligned == rows[group]
    np.add.at(by_aligned, (group, aligned), size)
    np.add.at(by_match, (group[is_core], match[is_core]), size[is_core])
    out = []
    for g, r in enumerate(rows.tolist()):
        a, m = by_aligned[g, 1:r + 1].tolist(), by_match[g, :r + 1].tolist()
        out.append({"covered": sum(a), "core": a[r - 1] if r else 0, "conserved": m[r] if r else 0, "by_aligned": a, "by_match": m})
    return out


def _conservation_parameters(k, rate, band, max_len, max_edits, ends):
    return (f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}, max_edits {int(max_edits)}" +
            (f", ends_max_len {int(ends[0])}, ends_max_edits {int(ends[1])}, ends_penalty {int(ends[2])}" if ends is not None else ""))


def conservation_bed(groups, segs, seg_first, k, rate, band, max_len, max_edits=0, ends=None):
    """The text of `<prefix>.block_conservation.bed`: a `#` line with the parameters, then one line per segment, CONSERVATION_BED_COLUMNS:
    the reference contig and bases [start, end), the block, the reference genome, the block's rows, and aligned, match, mismatch
    (aligned - match - gap) and gap.  groups: block_conservation's.  Columns are made as arrays and joined once per line.  Pure."""
    import numpy as np
    seg_first = np.asarray(seg_first, dtype=np.int64)
    group = np.repeat(np.arange(len(groups)), seg_first[1:] - seg_first[:-1])
    of_group = [np.array([str(g[f]) for g in groups], dtype=object)[group] if len(groups) else np.zeros(0, dtype=object) for f in (2, 0, 1, 5)]
    aligned, match, gap = (segs[f].astype(np.int64) for f in ("aligned", "match", "gap"))
    columns = [of_group[0], segs["start"].astype(np.int64), segs["end"].astype(np.int64), of_group[1], of_group[2], of_group[3], aligned, match,
               aligned - match - gap, gap]
    lines = ["\t".join(line) for line in zip(*(np.asarray(c).astype(str).tolist() for c in columns))]
    return "\n".join([_conservation_parameters(k, rate, band, max_len, max_edits, ends)] + lines) + "\n"


def conservation_table(groups, segs, seg_first, k, rate, band, max_len, max_edits=0, ends=None):
    """The text of `<prefix>.block_conservation.tsv`: a header, one line per block -- CONSERVATION_COLUMNS, the two histograms
    comma-joined, integers only -- then the `#` line with the parameters.  Pure."""
    summary = conservation_summary(segs, seg_first, [g[5] for g in groups])
    lines = ["\t".join(CONSERVATION_COLUMNS)]
    for g, s in zip(groups, summary):
        lines.append("\t".join([str(v) for v in g] + [str(s["covered"]), str(s["core"]), str(s["conserved"]), ",".join(map(str, s["by_aligned"])),
                                                      ",".join(map(str, s["by_match"]))]))
    lines.append(_conservation_parameters(k, rate, band, max_len, max_edits, ends))
    return "\n".join(lines) + "\n"


# ---- block variant sites: one allele table per block over the star alignment (docs/design/04_32_block_variant_sites.md) ----

VARIANT_SITES_COLUMNS = ("contig", "pos", "block_id", "genome", "type", "length", "ref", "alt", "rows", "aligned", "carriers", "genotypes")
VARIANT_SITE_TYPES = {1: "snv", 2: "del", 3: "ins"}


def alleles_host(entries, records, at, alt):
    """nts_cigar_alleles' alleles of ONE group on the host.  entries, records, at: that group's chains (the records' `first` index
    `entries`; the chains tile them); alt: their alt bytes, chain after chain (the X and I entries).  Events are made per entry with
    np.repeat, the insertions' bytes are gathered into one zero-padded matrix and numbered by np.unique over its rows, the alleles are
    np.unique over (pos, kind, len or alt byte, byte number) put into the device's order by their first event.  Returns (pos, kind, len,
    ref_off, alt_off, n_carriers, carriers): int64 arrays, one entry per allele but carriers, which holds every allele's chains one
    behind the other (indices into records); the offsets count inside this group's bytes.  Array operations over entries, events and
    bytes; the spot check of block_variant_sites and the baseline of scripts/block_variant_sites_measure.py.  Pure."""
    import numpy as np
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    alt = np.ascontiguousarray(alt, dtype=np.uint8)
    code, size = (entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64)
    n_cig, t0 = records["n_cig"].astype(np.int64), at["t0"].astype(np.int64)
    empty = np.zeros(0, dtype=np.int64)
    is_x, is_d, is_i = code == 8, code == 2, code == 1
    count = np.where(is_x, size, (is_d | is_i).astype(np.int64))
    n_ev = int(count.sum())
    if n_ev == 0:
        return empty, empty, empty, empty, empty, empty, empty
    chain_of = np.repeat(np.arange(n_cig.size), n_cig)        # (the chains tile the entries)
    first_of = np.concatenate(([0], np.cumsum(n_cig)))[chain_of]
    before = [np.concatenate(([0], np.cumsum(np.where(which, size, 0)))) for which in (~is_i, is_x | is_d, is_x | is_i)]   # A bases, ref bytes, alt bytes
    begin = t0[chain_of] + before[0][:-1] - before[0][first_of]
    ev_entry = np.repeat(np.arange(entries.size), count)
    off = np.where(is_x[ev_entry], np.arange(n_ev) - np.concatenate(([0], np.cumsum(count)))[ev_entry], 0)
    pos, kind = begin[ev_entry] + off, np.select([is_x[ev_entry], is_d[ev_entry]], [1, 2], 3)
    length = np.where(kind == 1, 1, size[ev_entry])
    ref_off = np.where(kind == 3, 0, before[1][ev_entry] + off)
    alt_off = np.where(kind == 2, 0, before[2][ev_entry] + off)
    what = np.zeros(n_ev, dtype=np.int64)                    # what tells events of one (pos, kind, len) apart: the alt byte, or the number of the bytes
    what[kind == 1] = alt[alt_off[kind == 1]]
    ins = np.flatnonzero(kind == 3)
    if ins.size:
        width = int(length[ins].max())
        column = np.arange(width)[None, :]
        padded = np.concatenate((alt, np.zeros(width, dtype=np.uint8)))
        text = np.where(column < length[ins][:, None], padded[np.minimum(alt_off[ins][:, None] + column, padded.size - 1)], 0)
        what[ins] = np.unique(text, axis=0, return_inverse=True)[1].reshape(-1)
    keys = np.stack((pos, kind, length, what), axis=1)
    _, lead, allele_of = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    allele_of = allele_of.reshape(-1)
    by_lead = np.where(kind[lead] == 1, what[lead], 0)       # (an SNV sorts by its byte, the others by their smallest carrier)
    order = np.lexsort((lead, by_lead, length[lead], kind[lead], pos[lead]))
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    lead = lead[order]
    events = np.argsort(rank[allele_of], kind="stable")
    return (pos[lead], kind[lead], length[lead], ref_off[lead], alt_off[lead], np.bincount(rank[allele_of], minlength=order.size).astype(np.int64),
            chain_of[ev_entry][events])


def variant_site_genotypes(alleles, carriers, chain_row, chain_t0, chain_t1, rows, chain_group):
    """Per allele one character per row 1 .. rows[group]: `1` a chain of that row carries the allele, `0` a chain of that row is aligned
    at it and does not carry it, `.` otherwise.  Aligned at: t0 <= pos < t1 for an SNV or DEL, t0 < pos < t1 for an INS.  alleles,
    carriers: nts_cigar_alleles'; chain_group, chain_row, chain_t0, chain_t1: per chain, the chains ascending by (group, row, t0) and
    those of one row not overlapping (as _star_cores orders and checks them); rows[g]: the rows of group g besides the reference.  ONE
    np.searchsorted over the keys (group, row, t0) for all alleles and rows.  Returns a list of strings.  Pure."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int64)
    chain_group, chain_row = np.asarray(chain_group, dtype=np.int64), np.asarray(chain_row, dtype=np.int64)
    chain_t0, chain_t1 = np.asarray(chain_t0, dtype=np.int64), np.asarray(chain_t1, dtype=np.int64)
    if alleles.size == 0:
        return []
    group, pos, kind = alleles["group"].astype(np.int64), alleles["pos"].astype(np.int64), alleles["kind"].astype(np.int64)
    most = int(rows.max()) if rows.size else 0
    big = int(max(chain_t1.max() if chain_t1.size else 0, pos.max())) + 2
    if (int(rows.size) * (most + 1) + most + 1) * big >= 1 << 62:
        raise ValueError("variant_site_genotypes: the keys (group, row, t0) leave 62 bits")
    keys = (chain_group * (most + 1) + chain_row) * big + chain_t0
    if np.any(keys[1:] < keys[:-1]):
        raise ValueError("variant_site_genotypes: the chains do not ascend by (group, row, t0)")
    row = np.arange(1, most + 1)[None, :]
    slot = (group[:, None] * (most + 1) + row)                 # [alleles, rows]
    at = np.searchsorted(keys, slot * big + pos[:, None], side="right") - 1
    hit = np.clip(at, 0, max(keys.size - 1, 0))
    found = (at >= 0) & (keys.size > 0)
    same = found & ((chain_group[hit] * (most + 1) + chain_row[hit]) == slot) if keys.size else found
    inside = same & (pos[:, None] < chain_t1[hit]) & ((kind[:, None] != 3) | (chain_t0[hit] < pos[:, None])) if keys.size else same
    out = np.where(inside, ord("0"), ord(".")).astype(np.uint8)
    out[row > rows[group][:, None]] = ord(" ")                # (beyond the group's rows: cut off below)
    n_car = alleles["n_carriers"].astype(np.int64)
    allele_of = np.repeat(np.arange(alleles.size), n_car)
    mine = np.asarray(carriers, dtype=np.int64)[(alleles["carrier_first"].astype(np.int64)[allele_of] + np.arange(allele_of.size) -
                                                 np.repeat(np.cumsum(n_car) - n_car, n_car))] if allele_of.size else np.zeros(0, dtype=np.int64)
    out[allele_of, chain_row[mine] - 1] = ord("1")
    return [line.tobytes().decode()[:r] for line, r in zip(out, rows[group].tolist())]


def variant_sites_table(groups, alleles, ref, alt, genotypes, k, rate, band, max_len, max_edits=0, ends=None):
    """The text of `<prefix>.block_variant_sites.tsv`: a header, one line per allele -- VARIANT_SITES_COLUMNS: the reference contig and
    0-based position, the block, the reference genome, snv / del / ins, the length, the reference's and the allele's letters (`-` for
    none), the block's rows, how many of them are aligned at the allele (the characters of `genotypes` that are no `.`), its carriers and
    the genotypes -- then the `#` line with the parameters.  groups: block_variant_sites'; ref, alt: the byte buffers the alleles' offsets
    count in.  Columns are made as arrays and joined once per line.  Pure."""
    import numpy as np
    ref_text, alt_text = np.asarray(ref, dtype=np.uint8).tobytes().decode(), np.asarray(alt, dtype=np.uint8).tobytes().decode()
    group, kind, length = alleles["group"].astype(np.int64), alleles["kind"].astype(np.int64).tolist(), alleles["len"].astype(np.int64).tolist()
    of_group = [np.array([str(g[f]) for g in groups], dtype=object)[group] if len(groups) else np.zeros(0, dtype=object) for f in (2, 0, 1, 5)]
    ref_of = [ref_text[o:o + n] if t != 3 else "-" for o, n, t in zip(alleles["ref_off"].tolist(), length, kind)]
    alt_of = [alt_text[o:o + n] if t != 2 else "-" for o, n, t in zip(alleles["alt_off"].tolist(), length, kind)]
    columns = [of_group[0], alleles["pos"].astype(np.int64), of_group[1], of_group[2], [VARIANT_SITE_TYPES[t] for t in kind], length, ref_of, alt_of,
               of_group[3], [len(g) - g.count(".") for g in genotypes], alleles["n_carriers"].astype(np.int64), genotypes]
    lines = ["\t".join(line) for line in zip(*(np.asarray(c, dtype=object).astype(str).tolist() for c in columns))]
    return "\n".join(["\t".join(VARIANT_SITES_COLUMNS)] + lines + [_conservation_parameters(k, rate, band, max_len, max_edits, ends)]) + "\n"


def _star_var_bases(ctx, genomes_by_name, blocks, held, entries, records):
    """The ref and alt bytes of _star_cores' chains in chain order, as nts_cigar_alleles and nts_cigar_profile take them: ONE
    nts_cigar_var_bases per pair of genomes over that pair's cores, the pairs' bytes scattered into chain order with one fancy-indexed
    store per pair and buffer.  Genomes given as callables are loaded for the bases, each query one at a time beside the reference's
    genome.  Returns (ref, ref_first, alt, alt_first): the bytes and where every chain's begin, the prefixes of the chains' X + D and
    X + I lengths (int64, len(held) + 1), which the device's firsts must agree with: RuntimeError."""
    import numpy as np
    from .device import CIG_SPAN_DTYPE
    code, size = (entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64)
    cut = np.concatenate((records["first"].astype(np.int64), [entries.size]))
    sums = [np.concatenate(([0], np.cumsum(np.where(np.isin(code, which), size, 0))))[cut] for which in ((8, 2), (8, 1))]
    ref_first, alt_first = sums                              # where every chain's bytes begin in chain order: prefixes of X + D and of X + I lengths
    ref, alt = np.zeros(int(ref_first[-1]), dtype=np.uint8), np.zeros(int(alt_first[-1]), dtype=np.uint8)
    by_pair = {}
    for j, h in enumerate(held):
        by_pair.setdefault((blocks[h[10]].genome, blocks[h[11]].genome), []).append(j)
    loaded = {}

    def genome(name):
        if name not in loaded:
            g = genomes_by_name[name]
            loaded[name] = (g(), True) if callable(g) else (g, False)
        return loaded[name][0]

    def release(name):
        g, mine = loaded.pop(name)
        if mine:
            g.free()
    try:
        for (name_a, name_b), members in by_pair.items():
            for name in [n for n in loaded if n not in (name_a, name_b)]:
                release(name)
            sub = records[members].copy()
            sub["first"] = np.concatenate(([0], np.cumsum(sub["n_cig"][:-1].astype(np.int64))))
            spans = np.zeros(len(members), dtype=CIG_SPAN_DTYPE)
            spans["pos_a"], spans["pos_b"] = [held[j][2] for j in members], [held[j][6] for j in members]
            spans["rec_a"], spans["rec_b"], spans["flags"] = [held[j][7] for j in members], [held[j][8] for j in members], [held[j][9] for j in members]
            mine = np.concatenate([held[j][3] for j in members]).astype(np.uint64)
            got = ctx.cigar_var_bases(mine, sub, spans, genome(name_a), genome(name_b))
            for whole, first, (part, part_first) in ((ref, ref_first, got[:2]), (alt, alt_first, got[2:])):
                part_first = part_first.astype(np.int64)
                sizes = part_first[1:] - part_first[:-1]
                if not np.array_equal(sizes, (first[1:] - first[:-1])[members]):
                    raise RuntimeError(f"the device's bytes per chain of {name_a} and {name_b} are not the X, D and I lengths of the chains")
                whole[np.repeat(first[:-1][members] - part_first[:-1], sizes) + np.arange(part.size)] = part     # (the scatter into chain order)
    finally:
        for name in list(loaded):
            release(name)
    return ref, ref_first, alt, alt_first


def block_variant_sites(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """Per synteny block the positions of its first line at which the other genomes differ, with which allele, and which of them share
    it (docs/design/04_32_block_variant_sites.md): the core chains of the star pairs (_star_cores) give, per pair of genomes, ONE
    nts_cigar_var_bases -- the bases at the X, D and I columns --, whose bytes are scattered into chain order, and ONE
    nts_cigar_alleles over all chains.  Genomes given as callables are loaded a second time for the bases, each query one at a time
    beside the reference's genome.  The first group's alleles and carriers are recomputed on the host (alleles_host) and compared:
    RuntimeError.  Returns (groups, alleles, ref, alt, genotypes): per block, in block_identity.tsv's order, (block_id, genome, contig,
    start, end, rows) of its first line; the CIG_ALLELE_DTYPE alleles in the device's order, the two byte buffers their offsets count in
    and variant_site_genotypes' strings: what variant_sites_table takes."""
    import numpy as np
    from .device import CIG_ALLELE_DTYPE
    n_groups, held, entries, records, at = _star_cores(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends)
    groups = [(b, blocks[lines[0]].genome, blocks[lines[0]].contig, blocks[lines[0]].start, blocks[lines[0]].end, len(lines) - 1)
              for b, lines in _block_order(blocks)]
    none = np.zeros(0, dtype=np.uint8)
    if not held:
        return groups, np.zeros(0, dtype=CIG_ALLELE_DTYPE), none, none, []
    ref, ref_first, alt, alt_first = _star_var_bases(ctx, genomes_by_name, blocks, held, entries, records)
    cut = np.concatenate((records["first"].astype(np.int64), [entries.size]))
    alleles, allele_first, carriers = ctx.cigar_alleles(entries, records, at, alt, n_groups)
    g0 = int(at["group"][0])                                  # the spot check: the first group that has chains
    mine = np.flatnonzero(at["group"] == g0)
    sub = records[mine].copy()
    sub["first"] -= records["first"][mine[0]]
    lo, hi = int(cut[mine[0]]), int(cut[mine[-1] + 1])
    host = alleles_host(entries[lo:hi], sub, at[mine], alt[int(alt_first[mine[0]]):int(alt_first[mine[-1] + 1])])
    got = alleles[int(allele_first[g0]):int(allele_first[g0 + 1])]
    want = list(host[:3]) + [np.where(host[1] == 3, 0, host[3] + ref_first[mine[0]]), np.where(host[1] == 2, 0, host[4] + alt_first[mine[0]]), host[5]]
    got_carriers = carriers[int(got["carrier_first"][0]):int(got["carrier_first"][-1]) + int(got["n_carriers"][-1])] if got.size else carriers[:0]
    if got.size != host[0].size or any(not np.array_equal(got[f].astype(np.int64), w) for f, w in zip(("pos", "kind", "len", "ref_off", "alt_off", "n_carriers"), want)) \
            or np.any(got["group"] != g0) or not np.array_equal(got_carriers.astype(np.int64), host[6] + mine[0]):
        raise RuntimeError(f"block {groups[g0][0]}: the device's {got.size} alleles differ from the host's {host[0].size}")
    t0 = at["t0"].astype(np.int64)
    genotypes = variant_site_genotypes(alleles, carriers, [h[1] for h in held], t0, t0 + records["len_a"].astype(np.int64), [g[5] for g in groups],
                                       at["group"].astype(np.int64))
    return groups, alleles, ref, alt, genotypes


# ---- block consensus: per-column profile and consensus over the star alignment (docs/design/04_33_block_consensus.md) ----

PROFILE_COLUMNS = ("contig", "pos", "sub", "block_id", "genome", "rows", "depth", "ref", "A", "C", "G", "T", "N", "gap", "call")
PROFILE_SYMBOLS = "ACGTN-"


def _profile_symbols(byte):
    "A C G T -> 0 .. 3, every other byte -> 4 (N), `-` -> 5: per element of a uint8 array"
    import numpy as np
    table = np.full(256, 4, dtype=np.int64)
    table[[ord(c) for c in "ACGT-"]] = [0, 1, 2, 3, 5]
    return table[np.asarray(byte, dtype=np.uint8)]


def _profile_tallies(cols):
    "[columns, 6] int64: the tallies of A C G T N - with the reference row counted in, as nts_cigar_profile's call reads them"
    import numpy as np
    from .device import CIG_PROFILE_REF
    tally = np.concatenate((cols["n"].astype(np.int64).reshape(-1, 5), cols["gap"].astype(np.int64)[:, None]), axis=1)
    is_ref = cols["sub"] == CIG_PROFILE_REF
    own = np.where(is_ref, np.minimum(_profile_symbols(cols["ref"]), 4), 5)          # (a reference byte that is no base counts under N)
    tally[np.arange(cols.size), own] += np.where(is_ref, cols["match"].astype(np.int64), 0) + 1
    return tally


def profile_host(entries, records, at, ref, alt):
    """nts_cigar_profile's columns of ONE group on the host.  entries, records, at: that group's chains (the records' `first` index
    `entries`; the chains tile them); ref, alt: their ref and alt bytes, chain after chain.  Events -- one per column of an X, D or I
    entry -- are made with np.repeat over the entries, `aligned` is a difference array over the group's reference extent, the
    per-symbol counts are np.unique over (pos, sub, symbol), the reference byte of a column is that of its first event (events are in
    chain order).  Returns a CIG_PROFILE_COL_DTYPE array in the device's order with group 0.  Array operations over entries, events
    and bases; the spot check of block_consensus and the baseline of scripts/block_consensus_measure.py.  Pure."""
    import numpy as np
    from .device import CIG_PROFILE_COL_DTYPE, CIG_PROFILE_REF
    entries = np.ascontiguousarray(entries, dtype=np.uint64)
    ref, alt = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(alt, dtype=np.uint8)
    code, size = (entries & np.uint64(15)).astype(np.int64), (entries >> np.uint64(4)).astype(np.int64)
    n_cig, t0, len_a = records["n_cig"].astype(np.int64), at["t0"].astype(np.int64), records["len_a"].astype(np.int64)
    is_x, is_d, is_i = code == 8, code == 2, code == 1
    count = np.where(is_x | is_d | is_i, size, 0)
    n_ev = int(count.sum())
    if n_ev == 0:
        return np.zeros(0, dtype=CIG_PROFILE_COL_DTYPE)
    chain_of = np.repeat(np.arange(n_cig.size), n_cig)        # (the chains tile the entries)
    first_of = np.concatenate(([0], np.cumsum(n_cig)))[chain_of]
    before = [np.concatenate(([0], np.cumsum(np.where(which, size, 0)))) for which in (~is_i, is_x | is_d, is_x | is_i)]   # A bases, ref bytes, alt bytes
    begin = t0[chain_of] + before[0][:-1] - before[0][first_of]
    ev_entry = np.repeat(np.arange(entries.size), count)
    off = np.arange(n_ev) - np.concatenate(([0], np.cumsum(count)))[ev_entry]
    ins, gone = is_i[ev_entry], is_d[ev_entry]
    pos = begin[ev_entry] + np.where(ins, 0, off)
    sub = np.where(ins, off, CIG_PROFILE_REF)
    symbol = np.full(n_ev, 5, dtype=np.int64)
    symbol[~gone] = np.minimum(_profile_symbols(alt[(before[2][ev_entry] + off)[~gone]]), 4)
    ref_at = before[1][ev_entry] + off                       # (of an X or D event)
    keys, counts = np.unique(np.stack((pos, sub, symbol), axis=1), axis=0, return_counts=True)
    columns, lead, of_column = np.unique(np.stack((pos, sub), axis=1), axis=0, return_index=True, return_inverse=True)
    column_of_key = np.unique(keys[:, :2], axis=0, return_inverse=True)[1].reshape(-1)
    held = np.zeros((columns.shape[0], 6), dtype=np.int64)
    held[column_of_key, keys[:, 2]] = counts
    r0, r1 = int(t0.min()), int((t0 + len_a).max())
    diff = np.zeros(r1 - r0 + 1, dtype=np.int64)
    np.add.at(diff, t0 - r0, 1)
    np.add.at(diff, t0 + len_a - r0, -1)
    aligned = np.cumsum(diff)[columns[:, 0] - r0]
    out = np.zeros(columns.shape[0], dtype=CIG_PROFILE_COL_DTYPE)
    is_ref = columns[:, 1] == CIG_PROFILE_REF
    out["pos"], out["sub"], out["aligned"] = columns[:, 0], columns[:, 1], aligned
    out["n"] = held[:, :5]
    out["gap"] = np.where(is_ref, held[:, 5], aligned - held[:, :5].sum(axis=1))
    out["match"] = np.where(is_ref, aligned - held.sum(axis=1), 0)
    out["ref"] = ord("-")
    if np.any(is_ref):
        out["ref"][is_ref] = ref[ref_at[lead[is_ref]]]
    tally = _profile_tallies(out)
    own = np.where(is_ref, np.minimum(_profile_symbols(out["ref"]), 4), 5)
    best = np.argmax(tally, axis=1)                           # (the first of A C G T N - among the largest)
    rows = np.arange(out.size)
    best = np.where(tally[rows, own] == tally[rows, best], own, best)
    out["call"] = np.frombuffer(PROFILE_SYMBOLS.encode(), dtype=np.uint8)[best]
    return out


def block_consensus(ctx, genomes_by_name, blocks, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None):
    """Per synteny block what the majority of its genomes hold at every variable column of its star alignment
    (docs/design/04_33_block_consensus.md): the core chains of the star pairs (_star_cores), their ref and alt bytes (_star_var_bases, as
    block_variant_sites makes them) and ONE nts_cigar_profile over all chains.  The columns of the first group that has chains are
    recomputed on the host (profile_host) and compared field by field: RuntimeError.  Returns (groups, cols, col_first, extents): per
    block, in block_identity.tsv's order, (block_id, genome, contig, start, end, rows) of its first line; the CIG_PROFILE_COL_DTYPE
    columns and where each block's begin; and per block (R0, R1), the smallest t0 and the largest t1 of its chains, None for a block
    without chains: what profile_table, consensus_reference_bases and consensus_fasta take."""
    import numpy as np
    from .device import CIG_PROFILE_COL_DTYPE
    n_groups, held, entries, records, at = _star_cores(ctx, genomes_by_name, blocks, k, rate, band, max_len, max_edits, ends)
    groups = [(b, blocks[lines[0]].genome, blocks[lines[0]].contig, blocks[lines[0]].start, blocks[lines[0]].end, len(lines) - 1)
              for b, lines in _block_order(blocks)]
    if not held:
        return groups, np.zeros(0, dtype=CIG_PROFILE_COL_DTYPE), np.zeros(n_groups + 1, dtype=np.uint64), [None] * n_groups
    ref, ref_first, alt, alt_first = _star_var_bases(ctx, genomes_by_name, blocks, held, entries, records)
    cols, col_first = ctx.cigar_profile(entries, records, at, ref, alt, n_groups)
    group_of, t0 = at["group"].astype(np.int64), at["t0"].astype(np.int64)
    t1 = t0 + records["len_a"].astype(np.int64)
    cut = np.searchsorted(group_of, np.arange(n_groups + 1))
    extents = [(int(t0[lo:hi].min()), int(t1[lo:hi].max())) if hi > lo else None for lo, hi in zip(cut[:-1].tolist(), cut[1:].tolist())]
    g0 = int(group_of[0])                                     # the spot check: the first group that has chains
    mine = np.arange(int(cut[g0]), int(cut[g0 + 1]))
    sub = records[mine].copy()
    sub["first"] -= records["first"][mine[0]]
    lo, hi = int(records["first"][mine[0]]), int(records["first"][mine[-1]] + records["n_cig"][mine[-1]])
    host = profile_host(entries[lo:hi], sub, at[mine], ref[int(ref_first[mine[0]]):int(ref_first[mine[-1] + 1])],
                        alt[int(alt_first[mine[0]]):int(alt_first[mine[-1] + 1])])
    got = cols[int(col_first[g0]):int(col_first[g0 + 1])]
    if got.size != host.size or np.any(got["group"] != g0) or \
            any(not np.array_equal(got[f], host[f]) for f in ("pos", "sub", "aligned", "match", "gap", "n", "ref", "call", "reserved")):
        raise RuntimeError(f"block {groups[g0][0]}: the device's {got.size} profile columns differ from the host's {host.size}")
    return groups, cols, col_first, extents


def consensus_reference_bases(genomes_by_name, groups, extents):
    """The upper-case reference bytes [R0, R1) of every group that has chains, None for the others: one read per group (_genome_bases)
    from the record named by the group's contig.  A genome given as a callable is loaded for its groups and freed behind them."""
    by_genome = {}
    for g, (group, extent) in enumerate(zip(groups, extents)):
        if extent is not None:
            by_genome.setdefault(group[1], []).append(g)
    out = [None] * len(groups)
    for name, members in by_genome.items():
        source = genomes_by_name[name]
        genome = source() if callable(source) else source
        try:
            record = {contig: r for r, contig in enumerate(genome.names)}
            for g in members:
                out[g] = _genome_bases(genome, record[groups[g][2]], extents[g][0], extents[g][1] - extents[g][0])
        finally:
            if callable(source):
                genome.free()
    return out


def consensus_sequences(groups, cols, col_first, extents, reference_bases):
    """Per group its reference bases [R0, R1) with the calls of its columns applied, as a str; None for a group without chains.
    reference_bases[g]: the upper-case bytes of the group's [R0, R1) (consensus_reference_bases).  A reference column whose call is a
    letter replaces the base, one whose call is `-` drops it; an insertion column whose call is a letter is inserted in front of base
    pos, in sub order, one whose call is `-` adds nothing; every other base keeps the reference's letter.  Array operations over one
    group's columns and bases: one np.insert and one mask per group.  Pure."""
    import numpy as np
    from .device import CIG_PROFILE_REF
    col_first = np.asarray(col_first, dtype=np.int64)
    out = []
    for g, extent in enumerate(extents):
        if extent is None:
            out.append(None)
            continue
        bases = np.array(reference_bases[g], dtype=np.uint8)
        if bases.size != extent[1] - extent[0]:
            raise ValueError(f"consensus_sequences: group {g} has {bases.size} reference bytes for [{extent[0]}, {extent[1]})")
        mine = cols[int(col_first[g]):int(col_first[g + 1])]
        at = mine["pos"].astype(np.int64) - extent[0]
        is_ref, gap = mine["sub"] == CIG_PROFILE_REF, mine["call"] == ord("-")
        keep = np.ones(bases.size, dtype=bool)
        bases[at[is_ref & ~gap]] = mine["call"][is_ref & ~gap]
        keep[at[is_ref & gap]] = False
        more = ~is_ref & ~gap                                 # (ascending by (pos, sub): np.insert keeps that order in front of one base)
        bases, keep = np.insert(bases, at[more], mine["call"][more]), np.insert(keep, at[more], True)
        out.append(bases[keep].tobytes().decode())
    return out


def consensus_fasta(groups, cols, col_first, extents, reference_bases):
    """The text of `<prefix>.block_consensus.fa`: per group that has chains, in block_identity.tsv's block order, the header
    `>block_<id> <genome>.<contig>:<R0>-<R1> rows=<rows> columns=<its emitted columns> changed=<those with call != ref>` and one
    unwrapped line, consensus_sequences' sequence.  Pure."""
    import numpy as np
    col_first = np.asarray(col_first, dtype=np.int64)
    lines = []
    for g, (group, extent, text) in enumerate(zip(groups, extents, consensus_sequences(groups, cols, col_first, extents, reference_bases))):
        if extent is None:
            continue
        mine = cols[int(col_first[g]):int(col_first[g + 1])]
        lines.append(f">block_{group[0]} {group[1]}.{group[2]}:{extent[0]}-{extent[1]} rows={group[5]} columns={mine.size} "
                     f"changed={int(np.count_nonzero(mine['call'] != mine['ref']))}")
        lines.append(text)
    return "\n".join(lines) + "\n" if lines else ""


def profile_table(groups, cols, col_first, k, rate, band, max_len, max_edits=0, ends=None):
    """The text of `<prefix>.block_profile.tsv`: a header, one line per column -- PROFILE_COLUMNS: the reference contig, the 0-based
    position, the column inside the slot in front of it (`.` for the reference base itself), the block, the reference genome, the
    block's rows, depth = aligned + 1, the reference's letter or `-`, the six tallies with the reference row counted in (they add up to
    depth) and the call -- then the `#` line with the parameters.  Integers only.  Columns are made as arrays and joined once per
    line.  Pure."""
    import numpy as np
    from .device import CIG_PROFILE_REF
    col_first = np.asarray(col_first, dtype=np.int64)
    group = np.repeat(np.arange(len(groups)), col_first[1:] - col_first[:-1])
    of_group = [np.array([str(g[f]) for g in groups], dtype=object)[group] if len(groups) else np.zeros(0, dtype=object) for f in (2, 0, 1, 5)]
    tally = _profile_tallies(cols)
    sub = np.where(cols["sub"] == CIG_PROFILE_REF, ".", cols["sub"].astype(np.int64).astype(str).astype(object))
    letters = [np.asarray(cols[f], dtype=np.uint8).tobytes().decode() for f in ("ref", "call")]
    columns = [of_group[0], cols["pos"].astype(np.int64), sub, of_group[1], of_group[2], of_group[3], cols["aligned"].astype(np.int64) + 1,
               list(letters[0])] + [tally[:, s] for s in range(6)] + [list(letters[1])]
    lines = ["\t".join(line) for line in zip(*(np.asarray(c, dtype=object).astype(str).tolist() for c in columns))]
    return "\n".join(["\t".join(PROFILE_COLUMNS)] + lines + [_conservation_parameters(k, rate, band, max_len, max_edits, ends)]) + "\n"


LIFT_COLUMNS = ("genome", "contig", "start", "end", "name", "block_id", "to_genome", "to_contig", "to_start", "to_end", "orientation", "ch", "src_start",
                "src_end", "status")
LIFT_IDENTITY_COLUMNS = LIFT_COLUMNS[:14] + ("matches", "mismatches", "src_gap_bases", "to_gap_bases", "src_gaps", "to_gaps", "columns", "identity", "status")
LIFT_STATS_FIELDS = ("eq", "x", "src_gap", "oth_gap", "src_gaps", "oth_gaps")       # of LIFT_STATS_DTYPE, in the order of the columns matches .. to_gaps


def read_bed(path):
    """The intervals of a BED3+ file, in file order: dict of contig and name (lists of str) and start, end (int64 arrays), 0-based and
    half-open.  Lines that begin with `#`, `track` or `browser` and empty lines are skipped; name is column 4, `.` when absent.  Fewer
    than 3 columns, a coordinate that is no integer or negative, or start >= end raise ValueError with the line's number."""
    import numpy as np
    contig, start, end, name = [], [], [], []
    with open(path, "r", encoding="utf-8") as fh:
        for number, line in enumerate(fh, 1):
            text = line.rstrip("\r\n")
            if not text.strip() or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            if len(f) < 3:
                raise ValueError(f"{path}, line {number}: a BED line has at least 3 columns (contig, start, end)")
            try:
                s, e = int(f[1]), int(f[2])
            except ValueError:
                raise ValueError(f"{path}, line {number}: start and end are integers") from None
            if s < 0 or e < 0:
                raise ValueError(f"{path}, line {number}: a negative coordinate")
            if s >= e:
                raise ValueError(f"{path}, line {number}: start {s} is not in front of end {e}")
            contig.append(f[0])
            start.append(s)
            end.append(e)
            name.append(f[3] if len(f) > 3 and f[3] else ".")
    return {"contig": contig, "name": name, "start": np.array(start, dtype=np.int64), "end": np.array(end, dtype=np.int64)}


def lift_queries(spans, intervals):
    """The join of the chains' source spans with the BED intervals, and the two queries of every overlap.  spans: dict, one entry per
    chain in which the source genome takes part, the chains of one pair next to each other and ascending by ch -- `pair` (any id of the
    pair), `chain` (the chain's index for nts_cigar_lift), `side` (0: the source is line a, the target; 1: line b, the query), `flip`
    (the pair is `-`), `contig` (the source contig, list of str) and `s0`, `s1`: the chain's forward span [S0, S1) on the source (side
    0: tstart, tend; side 1: qstart, qend of its PAF record).  intervals: read_bed's dict.  Every (interval, chain) pair of one contig
    with a non-empty overlap [lo, hi) = [max(start, S0), min(end, S1)) has the chain-local source offsets [u_lo, u_hi) = [lo - S0,
    hi - S0), but for side 1 of a `-` pair [S1 - hi, S1 - lo) (paf_row's mirroring, inverted), and makes two queries: pos = u_lo and
    pos = u_hi - 1.  Returns (queries, overlaps): a LIFT_QUERY_DTYPE array, overlap o's at 2 o and 2 o + 1, and a dict of int64 arrays
    interval, span (index into spans), lo, hi.  The chains of one pair are disjoint and ascending on both sides, so per pair the
    overlap ranges are two searchsorted and one np.repeat, over the intervals that can reach the pair alone (a contig's intervals are
    sorted by start once): a Python loop runs over pairs and contigs, never over intervals or queries."""
    import numpy as np
    from .device import LIFT_QUERY_DTYPE
    pair, s0, s1 = (np.asarray(spans[f], dtype=np.int64) for f in ("pair", "s0", "s1"))
    side, flip = np.asarray(spans["side"], dtype=np.int64), np.asarray(spans["flip"], dtype=bool)
    start, end = np.asarray(intervals["start"], dtype=np.int64), np.asarray(intervals["end"], dtype=np.int64)
    on_contig = {}                                            # source contig -> its intervals by start, those starts, the running maximum of their ends
    names = np.array(intervals["contig"], dtype=object)
    for c in set(spans["contig"]):
        mine = np.flatnonzero(names == c)
        mine = mine[np.argsort(start[mine], kind="stable")]
        on_contig[c] = (mine, start[mine], np.maximum.accumulate(end[mine]) if mine.size else end[mine])
    cuts = np.concatenate([[0], np.flatnonzero(pair[1:] != pair[:-1]) + 1, [pair.size]]) if pair.size else np.zeros(1, dtype=np.int64)
    which, span_of = [], []
    for lo_c, hi_c in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        order = np.arange(lo_c, hi_c)
        if hi_c - lo_c > 1 and s0[lo_c] > s0[lo_c + 1]:       # (side 1 of a `-` pair: ascending by ch is descending on the forward strand)
            order = order[::-1]
        if np.any(s0[order][1:] < s1[order][:-1]) or np.any(s0[order] > s1[order]):
            raise ValueError("the chains of a pair overlap on the source or are not in order")
        by_start, starts, ends_so_far = on_contig[spans["contig"][lo_c]]
        # the intervals that can reach the pair: from the first whose end, or an earlier one's, lies behind the pair's first base up to
        # the last that starts in front of the pair's end
        mine = by_start[np.searchsorted(ends_so_far, s0[order[0]], side="right"):np.searchsorted(starts, s1[order[-1]], side="left")]
        if mine.size == 0:
            continue
        first = np.searchsorted(s1[order], start[mine], side="right")          # the first chain that ends behind the interval's start
        last = np.searchsorted(s0[order], end[mine], side="left")              # the first chain that starts at or behind its end
        count = np.maximum(last - first, 0)
        total = int(count.sum())
        if total == 0:
            continue
        which.append(np.repeat(mine, count))
        span_of.append(order[np.repeat(first - np.concatenate([[0], np.cumsum(count)[:-1]]), count) + np.arange(total)])
    which = np.concatenate(which) if which else np.zeros(0, dtype=np.int64)
    span_of = np.concatenate(span_of) if span_of else np.zeros(0, dtype=np.int64)
    lo, hi = np.maximum(start[which], s0[span_of]), np.minimum(end[which], s1[span_of])
    keep = lo < hi                                            # (an empty chain overlaps nothing)
    which, span_of, lo, hi = which[keep], span_of[keep], lo[keep], hi[keep]
    mirrored = (side[span_of] == 1) & flip[span_of]
    u_lo = np.where(mirrored, s1[span_of] - hi, lo - s0[span_of])
    u_hi = np.where(mirrored, s1[span_of] - lo, hi - s0[span_of])
    queries = np.zeros(2 * which.size, dtype=LIFT_QUERY_DTYPE)
    queries["chain"] = np.repeat(np.asarray(spans["chain"], dtype=np.int64)[span_of], 2)
    queries["side"] = np.repeat(side[span_of], 2)
    queries["pos"][0::2], queries["pos"][1::2] = u_lo, u_hi - 1
    return queries, {"interval": which, "span": span_of, "lo": lo, "hi": hi}


def lift_rows(spans, overlaps, hits):
    """The lifted span of every overlap of lift_queries from its two hits L (of u_lo) and R (of u_hi - 1): on the other side of the
    chain [v_lo, v_hi) = [L.pos, R.pos + 1) when R's entry is `=` or `X`, else [L.pos, R.pos) -- R lies in a run the other side does not
    have, and R.pos is the first base behind it; an interval wholly inside such a run gives v_lo == v_hi.  With the chain's forward
    span [O0, O1) on the other genome (`o0`, `o1` of spans) the lifted span is [O0 + v_lo, O0 + v_hi), but for a `-` pair whose other
    side is line b [O1 - v_hi, O1 - v_lo).  Returns overlaps with to_start and to_end added.  v_lo > v_hi or a span that leaves
    [O0, O1) raises RuntimeError."""
    import numpy as np
    from .device import CIG_EQ, CIG_X
    span = overlaps["span"]
    left, right = hits[0::2], hits[1::2]
    v_lo = left["pos"].astype(np.int64)
    v_hi = right["pos"].astype(np.int64) + ((right["code"] == CIG_EQ) | (right["code"] == CIG_X))
    o0, o1 = np.asarray(spans["o0"], dtype=np.int64)[span], np.asarray(spans["o1"], dtype=np.int64)[span]
    if np.any(v_lo > v_hi) or np.any(v_hi > o1 - o0):
        raise RuntimeError("a lifted interval ends in front of its start or behind its chain")
    mirrored = (np.asarray(spans["side"], dtype=np.int64)[span] == 0) & np.asarray(spans["flip"], dtype=bool)[span]
    return dict(overlaps, to_start=np.where(mirrored, o1 - v_hi, o0 + v_lo), to_end=np.where(mirrored, o1 - v_lo, o0 + v_hi))


def lift_table(rows, k, rate, band, max_len, max_edits=0, ends=None, columns=LIFT_COLUMNS):
    """TSV of block_lift's rows: a header, one line per (interval, chain) overlap and one `unmapped` line per interval without any, then
    the footer with the parameters"""
    lines = ["\t".join(columns)] + ["\t".join(str(r[c]) for c in columns) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}, max_edits {int(max_edits)}" +
                 (f", ends_max_len {int(ends[0])}, ends_max_edits {int(ends[1])}, ends_penalty {int(ends[2])}" if ends is not None else ""))
    return "\n".join(lines) + "\n"


def lift_identity_table(rows, k, rate, band, max_len, max_edits=0, ends=None):
    "TSV of block_lift_identity's rows: LIFT_IDENTITY_COLUMNS; line order, status, the `unmapped` line and the footer are lift_table's"
    return lift_table(rows, k, rate, band, max_len, max_edits, ends, columns=LIFT_IDENTITY_COLUMNS)


def window_intervals(sizes, width):
    """The window grid of one genome in read_bed's shape: sizes = its contigs in FASTA order, (name, bases) pairs or a dict; per contig
    the intervals [0, W), [W, 2 W), ... with a shorter last one, named w0, w1, ... (counted per contig).  W < 1 raises ValueError.  A
    Python loop runs over contigs, never over windows."""
    import numpy as np
    width = int(width)
    if width < 1:
        raise ValueError(f"a window has at least one base (W = {width})")
    contig, name, start, end = [], [], [], []
    for c, bases in (sizes.items() if hasattr(sizes, "items") else sizes):
        s = np.arange(0, int(bases), width, dtype=np.int64)
        contig += [str(c)] * s.size
        name += np.char.add("w", np.arange(s.size).astype(str)).tolist()
        start.append(s)
        end.append(np.minimum(s + width, int(bases)))
    none = np.zeros(0, dtype=np.int64)
    return {"contig": contig, "name": name, "start": np.concatenate(start + [none]), "end": np.concatenate(end + [none])}


def lift_ranges(queries, overlaps, wanted=None):
    """One range per overlap of lift_queries, for nts_cigar_lift_stats: overlap o's two queries are pos = u_lo and pos = u_hi - 1 on one
    chain and side (the table of lift_queries), its range is (chain, side, u_lo, u_hi).  wanted: a bool per INTERVAL -- only the
    overlaps of those intervals get a range.  Returns (ranges, which): a LIFT_RANGE_DTYPE array and the overlaps they belong to.  Array
    operations alone."""
    import numpy as np
    from .device import LIFT_RANGE_DTYPE
    interval = np.asarray(overlaps["interval"], dtype=np.int64)
    if queries.size != 2 * interval.size:
        raise ValueError("lift_ranges: two queries per overlap")
    which = np.arange(interval.size) if wanted is None else np.flatnonzero(np.asarray(wanted, dtype=bool)[interval])
    ranges = np.zeros(which.size, dtype=LIFT_RANGE_DTYPE)
    ranges["chain"], ranges["side"] = queries["chain"][2 * which], queries["side"][2 * which]
    ranges["lo"], ranges["hi"] = queries["pos"][2 * which], queries["pos"][2 * which + 1] + np.uint64(1)
    return ranges, which


LIFT_JOINED_COLUMNS = LIFT_COLUMNS[:11] + ("chains", "first_ch", "last_ch", "src_start", "src_end", "matches", "mismatches", "src_gap_bases", "to_gap_bases",
                                           "src_gaps", "to_gaps", "src_open_bases", "to_open_bases", "columns", "identity", "status")
PAIR_STATS_FIELDS = ("eq", "x", "src_gap", "oth_gap", "src_gaps", "oth_gaps", "src_open", "oth_open")   # of PAIR_STATS_DTYPE, in the order of matches .. to_open_bases


def lift_pair_ranges(pairs, intervals):
    """The join of the pairs' source hulls with the intervals, for nts_cigar_lift_pairs.  pairs: dict, one entry per pair with a linked
    chain -- `side` (0: the source is line a, the target; 1: line b, the query), `flip` (the pair is `-`), `contig` (the source contig,
    list of str), `origin` (the source interval's start on the forward strand; for side 1 of a `-` pair its END: the pair's oriented
    offset u of a forward position p is p - origin, there origin - p, paf_row's mirroring) and `h0`, `h1`: the oriented hull [first
    link's start, last link's end) on the source side.  intervals: read_bed's dict.  Every (interval, pair) of one contig whose
    interval reaches the hull makes one range (pair, side, lo, hi): the interval in oriented offsets, mirrored inside the source
    interval where the offsets run backwards, clipped to the hull.  Returns (ranges, which): a PAIR_RANGE_DTYPE array with `pair` = the
    index into `pairs`, and the intervals they belong to.  Per pair two searchsorted over the contig's intervals (sorted by start
    once): a Python loop runs over pairs and contigs, never over intervals, chains or ranges."""
    import numpy as np
    from .device import PAIR_RANGE_DTYPE
    side, flip = np.asarray(pairs["side"], dtype=np.int64), np.asarray(pairs["flip"], dtype=bool)
    origin, h0, h1 = (np.asarray(pairs[f], dtype=np.int64) for f in ("origin", "h0", "h1"))
    start, end = np.asarray(intervals["start"], dtype=np.int64), np.asarray(intervals["end"], dtype=np.int64)
    mirrored = (side == 1) & flip
    f0, f1 = np.where(mirrored, origin - h1, origin + h0), np.where(mirrored, origin - h0, origin + h1)     # the hull on the forward strand
    on_contig = {}                                            # source contig -> its intervals by start, those starts, the running maximum of their ends
    names = np.array(intervals["contig"], dtype=object)
    for c in set(pairs["contig"]):
        mine = np.flatnonzero(names == c)
        mine = mine[np.argsort(start[mine], kind="stable")]
        on_contig[c] = (mine, start[mine], np.maximum.accumulate(end[mine]) if mine.size else end[mine])
    which, pair_of = [], []
    for p in range(side.size):
        if h0[p] >= h1[p]:
            continue
        by_start, starts, ends_so_far = on_contig[pairs["contig"][p]]
        mine = by_start[np.searchsorted(ends_so_far, f0[p], side="right"):np.searchsorted(starts, f1[p], side="left")]
        mine = np.sort(mine[end[mine] > f0[p]])
        which.append(mine)
        pair_of.append(np.full(mine.size, p, dtype=np.int64))
    which = np.concatenate(which) if which else np.zeros(0, dtype=np.int64)
    pair_of = np.concatenate(pair_of) if pair_of else np.zeros(0, dtype=np.int64)
    lo, hi = np.maximum(start[which], f0[pair_of]), np.minimum(end[which], f1[pair_of])      # (lo < hi: the interval reaches the hull)
    ranges = np.zeros(which.size, dtype=PAIR_RANGE_DTYPE)
    ranges["pair"], ranges["side"] = pair_of, side[pair_of]
    ranges["lo"] = np.where(mirrored[pair_of], origin[pair_of] - hi, lo - origin[pair_of])
    ranges["hi"] = np.where(mirrored[pair_of], origin[pair_of] - lo, hi - origin[pair_of])
    return ranges, which


def lift_joined_table(rows, k, rate, band, max_len, max_edits=0, ends=None):
    "TSV of block_lift_joined's rows: LIFT_JOINED_COLUMNS; line order, status, the `unmapped` line and the footer are lift_table's"
    return lift_table(rows, k, rate, band, max_len, max_edits, ends, columns=LIFT_JOINED_COLUMNS)


def chain_links(a):
    """(links, pair_first, base_x, base_y) of _chain_links, which see: what nts_cigar_lift_pairs and nts_cigar_chain_blocks take.  Pure."""
    return _chain_links(a)[:4]


def _chain_links(a):
    """The chains of one round of the alignment pass (an _AlignmentRound) as links for nts_cigar_lift_pairs and nts_cigar_chain_blocks:
    the chains with entries in (pair, ch) order at their oriented offsets x0, y0 -- moved per pair by base_x, base_y so that none is
    negative (a flank may leave the interval).  Returns (links, pair_first [lines + 1] int64, base_x, base_y [lines] int64, linked): link
    offset + base = alignment_pieces' offset; linked = the linked chains as indices into the chains sorted by line (stable), in link
    order.  Array operations alone.  Pure."""
    import numpy as np
    from .device import LIFT_LINK_DTYPE
    n_lines = len(a.round.lines)
    order = np.argsort(a.chains["line"], kind="stable")       # the chains of one pair next to each other, ascending by ch
    line = a.chains["line"][order]
    x0, y0 = a.chains["x0"][order], a.chains["y0"][order]
    linked = np.flatnonzero(np.asarray(a.records["n_cig"]).astype(np.int64)[order] > 0)   # (a chain without entries is not linked)
    linked = linked[np.lexsort((a.chains["ch"][order][linked], line[linked]))]              # link order: by pair, ascending by ch
    of_line = line[linked]
    pair_first = np.searchsorted(of_line, np.arange(n_lines + 1)).astype(np.int64)
    has = pair_first[1:] > pair_first[:-1]
    first = np.minimum(pair_first[:-1], max(linked.size - 1, 0))
    lx0, ly0 = x0[linked], y0[linked]
    base_x = np.where(has, np.minimum(lx0[first], 0), 0) if linked.size else np.zeros(n_lines, dtype=np.int64)
    base_y = np.where(has, np.minimum(ly0[first], 0), 0) if linked.size else np.zeros(n_lines, dtype=np.int64)
    links = np.zeros(linked.size, dtype=LIFT_LINK_DTYPE)
    links["chain"], links["a0"], links["b0"] = order[linked], lx0 - base_x[of_line], ly0 - base_y[of_line]
    return links, pair_first, base_x, base_y, linked


class _Lifter:
    """block_lift's state over the rounds of the alignment pass: per round the spans, ONE nts_cigar_lift and the rows' arrays.  stats: a
    bool per interval, or None -- per round also ONE nts_cigar_lift_stats for all overlaps of the intervals it marks (block_lift_identity).
    joined: a bool per interval, or None -- per round also ONE nts_cigar_lift_pairs for the intervals it marks and the pairs they reach
    (block_lift_joined); per_chain=False: that call alone, neither of the per-chain ones."""

    def __init__(self, genomes_by_name, blocks, source, intervals, stats=None, joined=None, per_chain=True):
        if source not in genomes_by_name:
            raise ValueError(f"--lift-genome {source} is not among the genomes {sorted(genomes_by_name)}")
        self.blocks, self.source, self.intervals, self.stats = blocks, source, intervals, stats
        self.joined, self.per_chain, self.joined_parts, self.joined_sorted = joined, per_chain, [], None
        if joined is not None:                                # the marked intervals, as lift_pair_ranges reads them, and which they are
            import numpy as np
            self.joined_which = np.flatnonzero(np.asarray(joined, dtype=bool))
            self.joined_intervals = {"contig": [intervals["contig"][j] for j in self.joined_which.tolist()],
                                     "start": np.asarray(intervals["start"], dtype=np.int64)[self.joined_which],
                                     "end": np.asarray(intervals["end"], dtype=np.int64)[self.joined_which]}
        self.contigs = None                                   # the source genome's records, once it was resident
        self.parts, self.info = [], {}                        # per round lift_rows' arrays with pair and ch; pair -> its columns
        self.index_of = None                                  # (line a, line b) -> the pair's place in block_identity's order
        self.sorted, self.sets = None, None                   # rows(): the parts in line order; _lifter_of: which intervals go to which table

    def add_round(self, ctx, a, pairs):
        import numpy as np
        r, chains = a.round, a.chains
        if self.source not in (r.name_a, r.name_b):
            return
        side = 0 if r.name_a == self.source else 1
        self.contigs = set((r.g_b if side else r.g_a).names)
        if self.index_of is None:                             # (`pairs` is complete before the first round)
            self.index_of = {p: q for q, p in enumerate(pairs)}
        index_of = self.index_of
        line = chains["line"]
        order = np.argsort(line, kind="stable")               # the chains of one pair next to each other, ascending by ch
        line = line[order]
        i = np.array([i for _, _, i in r.lines], dtype=np.int64)[line]
        start_a, start_b = r.iv_a[i, 1].astype(np.int64), r.iv_b[i, 1].astype(np.int64)
        end_b, flip = r.iv_b[i, 2].astype(np.int64), r.flip[i].astype(bool)
        x0, x1, y0, y1 = (chains[f][order] for f in ("x0", "x1", "y0", "y1"))
        t0, t1 = start_a + x0, start_a + x1                   # paf_row's tstart, tend, qstart, qend
        q0, q1 = np.where(flip, end_b - y1, start_b + y0), np.where(flip, end_b - y0, start_b + y1)
        pair = np.array([index_of[(la, lb)] for la, lb, _ in r.lines], dtype=np.int64)[line]
        mine = [self.blocks[(lb if side else la)].contig for la, lb, _ in r.lines]
        for q, (la, lb, _) in enumerate(r.lines):
            other = self.blocks[la if side else lb]
            self.info[index_of[(la, lb)]] = (self.blocks[la].block_id, other.genome, other.contig, "-" if self.blocks[la].strand != self.blocks[lb].strand else "+")
        spans = {"pair": pair, "chain": order, "side": np.full(order.size, side), "flip": flip, "contig": [mine[q] for q in line.tolist()],
                 "s0": q0 if side else t0, "s1": q1 if side else t1, "o0": t0 if side else q0, "o1": t1 if side else q1}
        if self.joined is not None:
            self._join_round(ctx, a, side, order, line, x0, x1, y0, y1, mine)
        if not self.per_chain:
            return
        queries, overlaps = lift_queries(spans, self.intervals)
        hits = ctx.cigar_lift(a.cigar, a.records, queries)    # (one call per round, for all pairs in which the source takes part)
        rows = lift_rows(spans, overlaps, hits)
        if self.stats is not None:
            from .device import CIG_EQ, CIG_X
            ranges, which = lift_ranges(queries, overlaps, self.stats)
            stats = ctx.cigar_lift_stats(a.cigar, a.records, ranges)                 # (one call per round, beside the lift's)
            left, right = hits[0::2][which], hits[1::2][which]
            both = stats["eq"] + stats["x"]
            if np.any(stats["oth_lo"] != left["pos"]) or np.any(stats["oth_hi"] != right["pos"] + np.isin(right["code"], (CIG_EQ, CIG_X))) or \
                    np.any(both + stats["src_gap"] != ranges["hi"] - ranges["lo"]) or np.any(both + stats["oth_gap"] != stats["oth_hi"] - stats["oth_lo"]):
                raise RuntimeError("the counts of a lifted interval do not add up to its two spans")
            for f in LIFT_STATS_FIELDS:                       # (-1: an overlap of an interval whose table has no counts)
                rows[f] = np.full(overlaps["interval"].size, -1, dtype=np.int64)
                rows[f][which] = stats[f].astype(np.int64)
        self.parts.append(dict(rows, pair=pair[rows["span"]], ch=chains["ch"][order][rows["span"]]))

    def _join_round(self, ctx, a, side, order, line, x0, x1, y0, y1, mine):
        """ONE nts_cigar_lift_pairs for the round: the chains with entries as links in (pair, ch) order at their oriented offsets -- moved
        per pair so that none is negative (a flank may leave the interval) --, one range per marked interval and pair whose hull it
        reaches (lift_pair_ranges); the records with a link, in forward coordinates, go to joined_parts"""
        import numpy as np
        r, n_lines = a.round, len(a.round.lines)
        links, pair_first, base_x, base_y, linked = _chain_links(a)
        has = pair_first[1:] > pair_first[:-1]
        first, last = np.minimum(pair_first[:-1], max(linked.size - 1, 0)), np.maximum(pair_first[1:] - 1, 0)
        lx0, lx1, ly0, ly1 = (v[linked] for v in (x0, x1, y0, y1))
        i = np.array([i for _, _, i in r.lines], dtype=np.int64)
        flip = r.flip[i].astype(bool) if n_lines else np.zeros(0, dtype=bool)
        origin_a = r.iv_a[i, 1].astype(np.int64) + base_x if n_lines else base_x
        origin_b = np.where(flip, r.iv_b[i, 2].astype(np.int64) - base_y, r.iv_b[i, 1].astype(np.int64) + base_y) if n_lines else base_y
        s0, s1 = (ly0, ly1) if side else (lx0, lx1)
        base = base_y if side else base_x
        hull = (np.where(has, s0[first] - base, 0), np.where(has, s1[last] - base, 0)) if linked.size else (base, base)
        pairs = {"side": np.full(n_lines, side), "flip": flip, "contig": mine, "origin": origin_b if side else origin_a, "h0": hull[0], "h1": hull[1]}
        ranges, which = lift_pair_ranges(pairs, self.joined_intervals)
        stats = ctx.cigar_lift_pairs(a.cigar, a.records, links, pair_first.astype(np.uint64), ranges)     # (one call per round, for all pairs of the source)
        keep = np.flatnonzero(stats["n_links"] > 0)
        st, q = stats[keep], ranges["pair"][keep].astype(np.int64)
        got = {f: st[f].astype(np.int64) for f in ("src_lo", "src_hi", "oth_lo", "oth_hi") + PAIR_STATS_FIELDS}
        both = got["eq"] + got["x"]
        if np.any(both + got["src_gap"] + got["src_open"] != got["src_hi"] - got["src_lo"]) or \
                np.any(both + got["oth_gap"] + got["oth_open"] != got["oth_hi"] - got["oth_lo"]):
            raise RuntimeError("the counts of a joined interval do not add up to its two spans")
        oa, ob, fl = origin_a[q], origin_b[q], flip[q]
        b_lo, b_hi = ("src_lo", "src_hi") if side else ("oth_lo", "oth_hi")         # which of the two spans lies on line b: mirrored for a `-` pair
        a_lo, a_hi = ("oth_lo", "oth_hi") if side else ("src_lo", "src_hi")
        on_a = (oa + got[a_lo], oa + got[a_hi])
        on_b = (np.where(fl, ob - got[b_hi], ob + got[b_lo]), np.where(fl, ob - got[b_lo], ob + got[b_hi]))
        src, to = (on_b, on_a) if side else (on_a, on_b)
        chs = a.chains["ch"][order][linked]
        index_of = self.index_of
        pair_id = np.array([index_of[(la, lb)] for la, lb, _ in r.lines], dtype=np.int64)
        part = {"interval": self.joined_which[which[keep]], "pair": pair_id[q], "chains": st["n_links"].astype(np.int64),
                "first_ch": chs[st["link_lo"].astype(np.int64)], "last_ch": chs[st["link_hi"].astype(np.int64)], "src_start": src[0], "src_end": src[1],
                "to_start": to[0], "to_end": to[1]}
        part.update({f: got[f] for f in PAIR_STATS_FIELDS})
        self.joined_parts.append(part)

    def _known_contigs(self, genomes_by_name):
        "every interval lies on a record of the source genome (ValueError otherwise)"
        if self.contigs is None:                              # (the source is in no pair: its records are read for the contig check alone)
            g = genomes_by_name[self.source]
            loaded = callable(g)
            g = g() if loaded else g
            self.contigs = set(g.names)
            if loaded:
                g.free()
        for c in dict.fromkeys(self.intervals["contig"]):
            if c not in self.contigs:
                raise ValueError(f"genome {self.source} has no record {c} (--block-lift)")

    def joined_rows(self, genomes_by_name, begin=0, end=None):
        "the lines of the intervals begin .. end - 1 (all) of the joined table: LIFT_JOINED_COLUMNS"
        import numpy as np
        self._known_contigs(genomes_by_name)
        iv = self.intervals
        fields = ("interval", "pair", "chains", "first_ch", "last_ch", "src_start", "src_end", "to_start", "to_end") + PAIR_STATS_FIELDS
        if self.joined_sorted is None:
            got = {f: np.concatenate([p[f] for p in self.joined_parts]) if self.joined_parts else np.zeros(0, dtype=np.int64) for f in fields}
            order = np.lexsort((got["pair"], got["interval"]))
            self.joined_sorted = {f: v[order] for f, v in got.items()}
        end = len(iv["contig"]) if end is None else end
        o, stop = (int(v) for v in np.searchsorted(self.joined_sorted["interval"], [begin, end]))
        got = {f: v[o:stop].tolist() for f, v in self.joined_sorted.items()}
        starts, ends, out, o, n = iv["start"].tolist(), iv["end"].tolist(), [], 0, stop - o
        absent = {c: "." for c in LIFT_JOINED_COLUMNS[5:-1]}
        for j in range(begin, end):
            head = {"genome": self.source, "contig": iv["contig"][j], "start": starts[j], "end": ends[j], "name": iv["name"][j]}
            if o == n or got["interval"][o] != j:
                out.append(dict(head, **absent, status="unmapped"))
            while o < n and got["interval"][o] == j:
                block_id, to_genome, to_contig, sign = self.info[got["pair"][o]]
                counts = [got[f][o] for f in PAIR_STATS_FIELDS]
                columns = sum(counts[:4])                     # (a link was reached: at least one column)
                v = (1000000 * counts[0]) // columns
                row = dict(head, block_id=block_id, to_genome=to_genome, to_contig=to_contig, to_start=got["to_start"][o], to_end=got["to_end"][o],
                           orientation=sign, chains=got["chains"][o], first_ch=got["first_ch"][o], last_ch=got["last_ch"][o], src_start=got["src_start"][o],
                           src_end=got["src_end"][o], columns=columns, identity=f"{v // 1000000}.{v % 1000000:06d}",
                           status="full" if (got["src_start"][o], got["src_end"][o]) == (starts[j], ends[j]) else "partial")
                row.update(zip(LIFT_JOINED_COLUMNS[16:24], counts))
                out.append(row)
                o += 1
        return out

    def rows(self, genomes_by_name, begin=0, end=None, identity=False):
        "the lines of the intervals begin .. end - 1 (all): LIFT_COLUMNS, or with identity LIFT_IDENTITY_COLUMNS"
        import numpy as np
        self._known_contigs(genomes_by_name)
        iv = self.intervals
        if self.sorted is None:
            fields = ("interval", "pair", "ch", "lo", "hi", "to_start", "to_end") + (LIFT_STATS_FIELDS if self.stats is not None else ())
            got = {f: np.concatenate([p[f] for p in self.parts]) if self.parts else np.zeros(0, dtype=np.int64) for f in fields}
            order = np.lexsort((got["ch"], got["pair"], got["interval"]))
            self.sorted = {f: v[order] for f, v in got.items()}
        end = len(iv["contig"]) if end is None else end
        o, stop = (int(v) for v in np.searchsorted(self.sorted["interval"], [begin, end]))
        got = {f: v[o:stop].tolist() for f, v in self.sorted.items()}
        starts, ends, out, o, n = iv["start"].tolist(), iv["end"].tolist(), [], 0, stop - o
        absent = {c: "." for c in (LIFT_IDENTITY_COLUMNS[5:-1] if identity else LIFT_COLUMNS[5:14])}
        for j in range(begin, end):
            head = {"genome": self.source, "contig": iv["contig"][j], "start": starts[j], "end": ends[j], "name": iv["name"][j]}
            if o == n or got["interval"][o] != j:
                out.append(dict(head, **absent, status="unmapped"))
            while o < n and got["interval"][o] == j:
                block_id, to_genome, to_contig, sign = self.info[got["pair"][o]]
                row = dict(head, block_id=block_id, to_genome=to_genome, to_contig=to_contig, to_start=got["to_start"][o], to_end=got["to_end"][o],
                           orientation=sign, ch=got["ch"][o], src_start=got["lo"][o], src_end=got["hi"][o],
                           status="full" if (got["lo"][o], got["hi"][o]) == (starts[j], ends[j]) else "partial")
                if identity:
                    counts = [got[f][o] for f in LIFT_STATS_FIELDS]
                    columns = sum(counts[:4])                 # (lo < hi: at least one column)
                    v = (1000000 * counts[0]) // columns
                    row.update(zip(LIFT_IDENTITY_COLUMNS[14:20], counts), columns=columns, identity=f"{v // 1000000}.{v % 1000000:06d}")
                out.append(row)
                o += 1
        return out

    def results(self, genomes_by_name):
        "(block_lift's rows or None, [block_lift_identity's rows per set]) of _lifter_of's sets"
        lift, identity = self.sets
        return (self.rows(genomes_by_name, *lift) if lift is not None else None, [self.rows(genomes_by_name, b, e, identity=True) for b, e in identity])


def _lifter_of(genomes_by_name, blocks, lift, lift_identity):
    """the _Lifter of one pass that serves block_lift's table (lift = (source, intervals) or None) and block_lift_identity's tables
    (lift_identity = (source, [intervals, ...])): the sets are joined as ONE list of intervals, so a round makes one nts_cigar_lift and one
    nts_cigar_lift_stats whatever the number of tables; a set that is the lift's own dict is joined once and read for both tables"""
    import numpy as np
    source, sets = lift_identity[0], list(lift_identity[1])
    if lift is not None and lift[0] != source:
        raise ValueError("the lift and the lift identity take the intervals of one genome")
    shared = [i for i, s in enumerate(sets) if lift is not None and s is lift[1]]
    every = ([lift[1]] if lift is not None and not shared else []) + sets
    cut = np.concatenate([[0], np.cumsum([len(s["contig"]) for s in every])]).tolist()
    spans = list(zip(cut[:-1], cut[1:]))
    stats = np.ones(cut[-1], dtype=bool)
    if lift is not None and not shared:
        stats[:cut[1]] = False
    intervals = {"contig": [c for s in every for c in s["contig"]], "name": [n for s in every for n in s["name"]],
                 "start": np.concatenate([np.asarray(s["start"], dtype=np.int64) for s in every]),
                 "end": np.concatenate([np.asarray(s["end"], dtype=np.int64) for s in every])}
    lifter = _Lifter(genomes_by_name, blocks, source, intervals, stats=stats)
    of_sets = spans[len(every) - len(sets):]
    lifter.sets = ((of_sets[shared[0]] if shared else spans[0]) if lift is not None else None, of_sets)
    return lifter


def record_sizes(genomes_by_name, source):
    "[(record, bases)] of the genome `source` in FASTA order, for window_intervals (a genome that is loaded for this alone is freed again)"
    if source not in genomes_by_name:
        raise ValueError(f"--lift-genome {source} is not among the genomes {sorted(genomes_by_name)}")
    g = genomes_by_name[source]
    loaded = callable(g)
    g = g() if loaded else g
    sizes = list(zip(g.names, (int(n) for n in g.rec_len)))
    if loaded:
        g.free()
    return sizes


def block_lift_identity(ctx, genomes_by_name, blocks, source, intervals, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN,
                        max_edits=0, ends=None, lift=None):
    """block_lift's lines with the alignment counts of every lifted interval: for every interval (read_bed's or window_intervals' dict) of
    the genome `source` and every chain it overlaps, the = and X columns, the bases either genome lacks and the runs of such bases between
    the columns of the clipped part's first and last base (nts_cigar_lift_stats; per round ONE call for all overlaps of all pairs,
    beside block_lift's nts_cigar_lift), as dicts of LIFT_IDENTITY_COLUMNS: columns = the sum of the four counts, identity =
    10^6 matches // columns as d.dddddd; an interval that overlaps no chain has `.` in block_id .. identity.  intervals: one dict, or a
    list of them -- then a list of row lists, from one pass.  lift: a dict of intervals (it may be one of `intervals`) whose block_lift
    rows the same pass makes as well; returns (those rows, the rows above).  docs/design/04_25_lift_identity.md."""
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        (check_ends_parameters(*(int(v) for v in ends)) if ends is not None else None)
    if message:
        raise ValueError(message)
    one = isinstance(intervals, dict)
    pairs, length = [], {}
    lifter = _lifter_of(genomes_by_name, blocks, (source, lift) if lift is not None else None, (source, [intervals] if one else intervals))
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, int(k), int(rate), int(band), int(max_len), int(max_edits), ends, pairs, length, only=source):
        lifter.add_round(ctx, a, pairs)
    lifted, identity = lifter.results(genomes_by_name)
    identity = identity[0] if one else identity
    return identity if lift is None else (lifted, identity)


def block_lifts(ctx, genomes_by_name, blocks, source, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN, max_edits=0, ends=None,
                lift=None, identity=(), joined=(), paf=False, cs=False, chain=False, maf=False):
    """Every table of the lift from ONE pass over _alignment_rounds, the joined ones among them: lift = a dict of intervals for block_lift's
    rows, identity = dicts for block_lift_identity's rows, joined = dicts for the joined rows (LIFT_JOINED_COLUMNS), paf: block_alignments'
    lines as well (cs: with the cs:Z: tag).  A dict that is given more than once is joined once and read for every table it serves.  The
    sets become ONE list of intervals, so a round makes at most one nts_cigar_lift, one nts_cigar_lift_stats and one
    nts_cigar_lift_pairs; the per-chain calls are made only when lift or identity asks for them.  Returns a dict: `paf` and `lift` (rows
    or None), `identity` and `joined` (a list of rows per set)."""
    import numpy as np
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        (check_ends_parameters(*(int(v) for v in ends)) if ends is not None else None)
    if message:
        raise ValueError(message)
    every = []

    def place(one):
        for at, other in enumerate(every):
            if other is one:
                return at
        every.append(one)
        return len(every) - 1
    at_lift = place(lift) if lift is not None else None
    at_identity, at_joined = [place(one) for one in identity], [place(one) for one in joined]
    cut = np.concatenate([[0], np.cumsum([len(one["contig"]) for one in every])]).astype(np.int64).tolist()
    spans = list(zip(cut[:-1], cut[1:]))
    counted, joining = np.zeros(cut[-1], dtype=bool), np.zeros(cut[-1], dtype=bool)
    for mask, places in ((counted, at_identity), (joining, at_joined)):
        for at in places:
            mask[spans[at][0]:spans[at][1]] = True
    intervals = {"contig": [c for one in every for c in one["contig"]], "name": [n for one in every for n in one["name"]],
                 "start": np.concatenate([np.asarray(one["start"], dtype=np.int64) for one in every] + [np.zeros(0, dtype=np.int64)]),
                 "end": np.concatenate([np.asarray(one["end"], dtype=np.int64) for one in every] + [np.zeros(0, dtype=np.int64)])}
    lifter = _Lifter(genomes_by_name, blocks, source, intervals, stats=counted if at_identity else None, joined=joining if at_joined else None,
                     per_chain=lift is not None or bool(at_identity))
    pairs, length, found, chains_of, mafs_of = [], {}, {}, {}, {}
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, int(k), int(rate), int(band), int(max_len), int(max_edits), ends, pairs, length,
                               only=None if paf or chain or maf else source, cs=bool(cs) and bool(paf), maf=bool(maf)):
        if paf:
            _round_paf_rows(blocks, a, found)
        lifter.add_round(ctx, a, pairs)
        if chain:
            _round_chain_parts(ctx, blocks, a, chains_of)
        if maf:
            _round_maf_parts(blocks, a, mafs_of)
    return {"chain": [chains_of[p] for p in pairs if chains_of.get(p) is not None] if chain else None,   # (chain: block_chains' parts from the same pass)
            "maf": [part for p in pairs for part in mafs_of[p]] if maf else None,                      # (maf: block_mafs' parts from the same pass)
            "paf": [row for p in pairs for row in found[p]] if paf else None,
            "lift": lifter.rows(genomes_by_name, *spans[at_lift]) if lift is not None else None,
            "identity": [lifter.rows(genomes_by_name, *spans[at], identity=True) for at in at_identity],
            "joined": [lifter.joined_rows(genomes_by_name, *spans[at]) for at in at_joined]}


def block_lift_joined(ctx, genomes_by_name, blocks, source, intervals, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN,
                      max_edits=0, ends=None):
    """One line per interval and PAIR of block lines: for every interval (read_bed's or window_intervals' dict) of the genome `source`
    and every pair in which it reaches a chain, the span joined across the pair's chains -- from the first to the last base of the
    interval that a chain holds --, the alignment counts over every column between the two, the chains between them whole, and the bases
    of the stretches between the chains that no column covers (nts_cigar_lift_pairs; per round ONE call for all intervals and pairs, and
    no per-chain call), as dicts of LIFT_JOINED_COLUMNS: chains = the chains reached, first_ch / last_ch their numbers, columns = the
    sum of the four counts, identity = 10^6 matches // columns as d.dddddd; an interval that reaches no chain has `.` in block_id ..
    identity and status `unmapped`.  docs/design/04_27_lift_joined.md."""
    import numpy as np
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        (check_ends_parameters(*(int(v) for v in ends)) if ends is not None else None)
    if message:
        raise ValueError(message)
    pairs, length = [], {}
    lifter = _Lifter(genomes_by_name, blocks, source, intervals, joined=np.ones(len(intervals["contig"]), dtype=bool), per_chain=False)
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, int(k), int(rate), int(band), int(max_len), int(max_edits), ends, pairs, length, only=source):
        lifter.add_round(ctx, a, pairs)
    return lifter.joined_rows(genomes_by_name)


def block_lift(ctx, genomes_by_name, blocks, source, intervals, k=IDENTITY_K, rate=IDENTITY_RATE, band=IDENTITY_BAND, max_len=IDENTITY_MAX_LEN,
               max_edits=0, ends=None):
    """read_bed's intervals of the genome `source` mapped through the block alignments: for every interval and every chain of
    block_alignments (same parameters, same pass: _alignment_rounds) whose source span it overlaps, the clipped part [src_start,
    src_end) and where its first and its last base lie in the other genome of the pair, from the chain's CIGAR (nts_cigar_lift; per
    round ONE call for all queries of all pairs in which `source` takes part, on either line).  Returns dicts of LIFT_COLUMNS: the
    intervals in input order, per interval the pairs in block_identity's order and a pair's chains ascending by ch; status `full` when
    nothing was clipped, else `partial`; an interval that overlaps no chain has one line, `.` in block_id .. src_end and status
    `unmapped`.  An interval on a contig the genome does not have raises ValueError.  docs/design/04_23_block_lift.md."""
    message = check_identity_parameters(int(k), int(rate), int(band), int(max_len), int(max_edits)) or \
        (check_ends_parameters(*(int(v) for v in ends)) if ends is not None else None)
    if message:
        raise ValueError(message)
    pairs, length = [], {}
    lifter = _Lifter(genomes_by_name, blocks, source, intervals)
    for a in _alignment_rounds(ctx, genomes_by_name, blocks, int(k), int(rate), int(band), int(max_len), int(max_edits), ends, pairs, length, only=source):
        lifter.add_round(ctx, a, pairs)
    return lifter.rows(genomes_by_name)


def wide_variants_table(rows, k, rate, band, max_len, max_edits):
    """TSV of block_wide_variants' variant rows: the columns and the order of variants_table, every event of every aligned stretch,
    narrow and wide, then `# k K, rate R, band W, max_len L, max_edits E`"""
    lines = ["\t".join(VARIANT_COLUMNS)] + [variant_row(r) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}, max_edits {int(max_edits)}")
    return "\n".join(lines) + "\n"


def variant_events(ops, segs, start_a, start_b, len_b, flipped):
    """The events of one pair of lines.  ops: OP_DTYPE entries in script order whose `seg` indexes segs (SEGMENT_DTYPE); start_a /
    start_b: the clipped interval starts within their records, len_b: B's clipped length.  A maximal run of adjacent DEL ops with
    consecutive p and one q is one `del`, a maximal run of adjacent INS ops with one p and consecutive q one `ins`, every SUB an
    `snv`.  Returns dicts of type, pos_a, pos_b, length, seq_a, seq_b (0-based positions on the forward strand of the records; seq_b in
    the oriented frame; `-` for no bases; the side without bases has the position of the base that follows in the oriented frame),
    ascending by pos_a, then in script order.  Pure."""
    sub, dele, ins = 1, 2, 3
    runs = []                                                 # [seg, op, p0, q0, bases of A, bases of B]
    for seg, p, q, op, base_a, base_b, _ in (ops.tolist() if hasattr(ops, "tolist") else ops):
        if op not in (sub, dele, ins) or (op != ins and base_a > 3) or (op != dele and base_b > 3):
            raise ValueError(f"not an edit op: {(seg, p, q, op, base_a, base_b)}")
        last = runs[-1] if runs else None
        if last and last[0] == seg and last[1] == op == dele and p == last[2] + len(last[4]) and q == last[3]:
            last[4] += "ACGT"[base_a]
        elif last and last[0] == seg and last[1] == op == ins and p == last[2] and q == last[3] + len(last[5]):
            last[5] += "ACGT"[base_b]
        else:
            runs.append([seg, op, p, q, "" if op == ins else "ACGT"[base_a], "" if op == dele else "ACGT"[base_b]])
    out = []
    for seg, op, p0, q0, seq_a, seq_b in runs:
        y = int(segs[seg]["y_lo"]) + q0
        out.append({"type": {sub: "snv", dele: "del", ins: "ins"}[op], "pos_a": start_a + int(segs[seg]["x"]) + p0,
                    "pos_b": start_b + len_b - y - len(seq_b) if flipped else start_b + y, "length": max(len(seq_a), len(seq_b)),
                    "seq_a": seq_a or "-", "seq_b": seq_b or "-"})
    out.sort(key=lambda e: e["pos_a"])                        # (stable: script order within one position)
    return out


def variant_row(r):
    "one line of the variants table"
    return "\t".join(str(r[c]) for c in VARIANT_COLUMNS)


def variants_table(rows, k, rate, band, max_len):
    "TSV with a header, one line per event, then `# k K, rate R, band W, max_len L`"
    lines = ["\t".join(VARIANT_COLUMNS)] + [variant_row(r) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}")
    return "\n".join(lines) + "\n"


def identity_row(r):
    """one line of the identity table, integer arithmetic throughout: identity = (10^6 (M - edits)) // M with M the larger of the two
    aligned lengths, six decimals, `.` for M = 0; covered_* = (1000 aligned) // length as per cent with one decimal, `.` for length 0"""
    m = max(r["aligned_a"], r["aligned_b"])
    if m == 0:
        identity = "."
    else:
        v = (1000000 * (m - r["edits"])) // m
        identity = f"{v // 1000000}.{v % 1000000:06d}"

    def covered(aligned, length):
        if length == 0:
            return "."
        v = (1000 * aligned) // length
        return f"{v // 10}.{v % 10}"
    shown = dict(r, identity=identity, covered_a=covered(r["aligned_a"], r["length_a"]), covered_b=covered(r["aligned_b"], r["length_b"]))
    return "\t".join(str(shown[c]) for c in IDENTITY_COLUMNS)


def identity_table(rows, k, rate, band, max_len, max_edits=0):
    "TSV with a header, one line per block and pair of its lines, then `# k K, rate R, band W, max_len L` -- and `, max_edits E` for E > 0"
    lines = ["\t".join(IDENTITY_COLUMNS)] + [identity_row(r) for r in rows]
    lines.append(f"# k {int(k)}, rate {int(rate)}, band {int(band)}, max_len {int(max_len)}" + (f", max_edits {int(max_edits)}" if int(max_edits) else ""))
    return "\n".join(lines) + "\n"


def main(argv=None):
    "bin/ntsynt_block_stats"
    import argparse
    p = argparse.ArgumentParser(prog="ntsynt_block_stats", description="Summary statistics of a synteny block table (number of blocks, coverage, "
                                "mean / median length, NG50, N50) and, with --fastas, the Mash distance of every block per pair of its genomes (GPU)")
    p.add_argument("--tsv", help="synteny block table (<prefix>.synteny_blocks.tsv)", required=True)
    p.add_argument("--fai", help=".fai files of the compared genomes", nargs="+", required=True)
    p.add_argument("--fastas", help="the genomes themselves: per-block divergence on the GPU (matched to column 2 of the table by base name)",
                   nargs="+")
    p.add_argument("-k", help=f"k-mer size of the sketches [{K_DEFAULT}]", type=int, default=K_DEFAULT)
    p.add_argument("-s", help=f"sketch size [{S_DEFAULT}]", type=int, default=S_DEFAULT)
    p.add_argument("--divergence-out", help="file for the per-block table [stdout, after the statistics]")
    p.add_argument("--identity-out", help="with --fastas: file for the per-block identity table (exact edit distance between anchors; GPU)")
    p.add_argument("--variants-out", help="with --fastas: file for the per-block variants table (the edits behind the identity table's `edits`, as snv / ins / "
                   "del events in both genomes' coordinates; GPU); it takes the --identity-* parameters")
    p.add_argument("--wide-variants-out", help="with --fastas and --identity-max-edits E > 0: file for the complete per-block variants table, the events of "
                   "the stretches the band leaves out (indels of 32 bases or more) included; GPU; it takes the --identity-* parameters")
    p.add_argument("--identity-k", help=f"k-mer size of the anchors [{IDENTITY_K}]", type=int, default=IDENTITY_K)
    p.add_argument("--identity-rate", help=f"sample one in this many k-mers as anchor candidates [{IDENTITY_RATE}]", type=int, default=IDENTITY_RATE)
    p.add_argument("--identity-band", help=f"half-width of the alignment band, 1..31 [{IDENTITY_BAND}]", type=int, default=IDENTITY_BAND)
    p.add_argument("--identity-max-len", help=f"longest stretch between two anchors that is aligned, 1..65535 [{IDENTITY_MAX_LEN}]", type=int,
                   default=IDENTITY_MAX_LEN)
    p.add_argument("--identity-max-edits", help="with --identity-out or --wide-variants-out (which needs it): also align the stretches the band leaves "
                   "out (indels of 32 bases or more), up to this many edits: 0 = off, else 2 * --identity-band + 1 .. 1023; not with "
                   "--variants-out [0]", type=int, default=0)
    p.add_argument("--ends-out", help="with --fastas: file for the per-block ends table (the base-exact breakpoints of every block and pair: how far the "
                   "alignment continues beyond the first and the last aligned stretch; GPU); it takes the --identity-* parameters")
    p.add_argument("--end-variants-out", help="with --ends-out (which it needs): file for the per-block end variants table (the edits behind left_edits and "
                   "right_edits of the ends table, as snv / ins / del events in both genomes' coordinates; GPU)")
    p.add_argument("--paf-out", help="with --fastas: file for the block alignments (one PAF record with a cg:Z: CIGAR per aligned chain of every block and "
                   "pair; GPU); it takes the --identity-* parameters, --identity-max-edits included, and with --ends-out the --ends-* parameters: the "
                   "flanks are attached")
    p.add_argument("--paf-cs", help="with --paf-out (which it needs): every record also carries the cs:Z: tag (short form) behind cg:Z:; both tag texts "
                   "are then made on the GPU", action="store_true")
    p.add_argument("--chain-out", help="with --fastas: file for the block chain file (one UCSC liftover chain per block and pair, the chains of --paf-out "
                   "joined per pair with the stretches between them as dt dq gaps; GPU); it takes the parameters of --paf-out")
    p.add_argument("--maf-out", help="with --fastas: file for the block MAF (one pairwise MAF block per record of --paf-out with both aligned rows, made on "
                   "the GPU); it takes the parameters of --paf-out; a pass of its own")
    p.add_argument("--multi-maf-out", help="with --fastas: file for the block multi-MAF (one reference-anchored multiple alignment per synteny block, anchored "
                   "on the block's first line, cut into sub-blocks where the covering genomes change; padded CIGARs and rows made on the GPU); it takes "
                   "the parameters of --paf-out; a pass of its own, which loads each query genome a second time for the rows")
    p.add_argument("--conservation-out", help="with --fastas and --conservation-stats-out: file for the block conservation segments (BED: per synteny "
                   "block the runs of bases of its first line with one aligned / match / mismatch / gap count over the star alignment of "
                   "--multi-maf-out; made on the GPU); it takes the parameters of --paf-out; a pass of its own")
    p.add_argument("--conservation-stats-out", help="with --conservation-out: file for the per-block table (covered, core and conserved bases, histograms)")
    p.add_argument("--variant-sites-out", help="with --fastas: file for the block variant sites (per synteny block one line per allele over the star "
                   "alignment of --multi-maf-out: position on the block's first line, snv / del / ins, the letters, the carriers and one genotype "
                   "character per row; bases and allele table made on the GPU); it takes the parameters of --paf-out; a pass of its own")
    p.add_argument("--profile-out", help="with --fastas and --consensus-out: file for the block profile (per synteny block one line per variable column "
                   "of the star alignment of --multi-maf-out, reference bases and insertion columns alike: the tallies of A C G T N and the gap with "
                   "the reference row counted in, and the plurality call; made on the GPU); it takes the parameters of --paf-out; a pass of its own")
    p.add_argument("--consensus-out", help="with --profile-out: file for the block consensus (FASTA: per synteny block its first line's bases with the "
                   "calls applied)")
    p.add_argument("--lift-bed", help="with --fastas, --lift-genome and --lift-out: a BED file of intervals of one genome that are mapped through the block "
                   "alignments into the other genomes (GPU); it takes the parameters of --paf-out")
    p.add_argument("--lift-genome", help="the genome the intervals of --lift-bed lie on: a FASTA base name, as in column 2 of the block table")
    p.add_argument("--lift-out", help="file for the lifted intervals (one line per interval and aligned chain it overlaps)")
    p.add_argument("--lift-identity-out", help="with --lift-bed and --lift-genome: file for the lifted intervals with their alignment counts (matches, "
                   "mismatches, the bases either genome lacks, identity; GPU)")
    p.add_argument("--lift-windows", help="with --lift-genome and --lift-windows-out: the same counts for windows of this many bases over every record "
                   "of that genome", type=int)
    p.add_argument("--lift-windows-out", help="file for the windows of --lift-windows")
    p.add_argument("--lift-joined-out", help="with --lift-bed and --lift-genome: file for the intervals joined per pair of block lines (one line per "
                   "interval and pair: the span across the pair's chains, its counts and the bases between the chains; GPU)")
    p.add_argument("--lift-windows-joined-out", help="with --lift-windows and --lift-genome: the same joined table for the windows")
    p.add_argument("--ends-max-len", help=f"longest flank that is extended, 1..65535 [{ENDS_MAX_LEN}]", type=int, default=ENDS_MAX_LEN)
    p.add_argument("--ends-max-edits", help=f"most edits within one flank, 1..1023 [{ENDS_MAX_EDITS}]", type=int, default=ENDS_MAX_EDITS)
    p.add_argument("--ends-penalty", help=f"what an edit costs the extension's score, against 2 for a matching pair of bases, 3..255 [{ENDS_PENALTY}]",
                   type=int, default=ENDS_PENALTY)
    p.add_argument("--device", help="GPU index [0]", type=int, default=0)
    args = p.parse_args(argv)
    if args.k < 1 or args.s < 1:
        p.error("-k and -s must be positive")
    if args.end_variants_out and not args.ends_out:
        p.error("--end-variants-out: " + END_VARIANTS_NEED_ENDS)
    if args.ends_out:
        if not args.fastas:
            p.error("--ends-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits) or \
            check_ends_parameters(args.ends_max_len, args.ends_max_edits, args.ends_penalty)
        if message:
            p.error(message)
    if args.paf_out:
        if not args.fastas:
            p.error("--paf-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.chain_out:
        if not args.fastas:
            p.error("--chain-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.multi_maf_out:
        if not args.fastas:
            p.error("--multi-maf-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if bool(args.conservation_out) != bool(args.conservation_stats_out):
        p.error("--conservation-out and --conservation-stats-out go together")
    if args.conservation_out:
        if not args.fastas:
            p.error("--conservation-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.variant_sites_out:
        if not args.fastas:
            p.error("--variant-sites-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if bool(args.profile_out) != bool(args.consensus_out):
        p.error("--profile-out and --consensus-out go together")
    if args.profile_out:
        if not args.fastas:
            p.error("--profile-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.maf_out:
        if not args.fastas:
            p.error("--maf-out needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.paf_cs and not args.paf_out:
        p.error("--paf-cs adds the cs:Z: tag to the records of --paf-out: it needs that switch")
    if args.lift_identity_out and not args.lift_bed:
        p.error("--lift-identity-out needs the intervals: --lift-bed (and --lift-genome)")
    if args.lift_joined_out and not (args.lift_bed and args.lift_genome):
        p.error("--lift-joined-out needs the intervals and their genome: --lift-bed and --lift-genome")
    if args.lift_windows_joined_out and args.lift_windows is None:
        p.error("--lift-windows-joined-out needs the windows: --lift-windows W (and --lift-genome)")
    if (args.lift_windows is not None) != bool(args.lift_windows_out or args.lift_windows_joined_out):
        p.error("--lift-windows and --lift-windows-out go together")
    if args.lift_windows is not None:
        if not args.lift_genome:
            p.error("--lift-windows needs --lift-genome: the genome the windows lie on")
        if args.lift_windows < 1:
            p.error("--lift-windows: a window has at least one base")
    if args.lift_bed or args.lift_genome or args.lift_out:
        if not (args.lift_genome and (args.lift_windows_out or args.lift_windows_joined_out or
                                      (args.lift_bed and (args.lift_out or args.lift_identity_out or args.lift_joined_out))) and
                bool(args.lift_bed) == bool(args.lift_out or args.lift_identity_out or args.lift_joined_out)):
            p.error("--lift-bed, --lift-genome and --lift-out go together")
        if not args.fastas:
            p.error("--lift-out needs the genomes: --fastas")
        if args.lift_genome not in [os.path.basename(path) for path in args.fastas]:
            p.error(f"--lift-genome {args.lift_genome} is not among the genomes {[os.path.basename(path) for path in args.fastas]}")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
    if args.identity_out or args.variants_out or args.wide_variants_out:
        if not args.fastas:
            p.error(("--identity-out" if args.identity_out else "--variants-out" if args.variants_out else "--wide-variants-out") +
                    " needs the genomes: --fastas")
        message = check_identity_parameters(args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len, args.identity_max_edits)
        if message:
            p.error(message)
        if args.identity_max_edits and args.variants_out:
            p.error(WIDE_NOT_WITH_VARIANTS)
        if args.wide_variants_out and not args.identity_max_edits:
            p.error("--wide-variants-out: " + WIDE_VARIANTS_NEED_E)
    print(stats_table(block_stats(args.tsv, args.fai)), end="")
    if not args.fastas:
        return 0
    for path in args.fastas:
        if not os.path.isfile(path):
            raise FileNotFoundError(f"Input file {path} not found.")
    from .device import Context
    from .fasta import basename, read_fasta_device
    ctx = Context(args.device)
    try:
        loaders = {basename(path): (lambda path=path: read_fasta_device(ctx, path)[0]) for path in args.fastas}
        text = divergence_table(block_divergence(ctx, loaders, read_blocks(args.tsv), args.k, args.s), args.k, args.s)
        id_args = (args.identity_k, args.identity_rate, args.identity_band, args.identity_max_len)
        chain_parts = None
        if args.variants_out:                                 # (one pass gives both tables)
            id_rows, var_rows = block_variants(ctx, loaders, read_blocks(args.tsv), *id_args)
            with open(args.variants_out, "w", encoding="utf-8") as fh:
                fh.write(variants_table(var_rows, *id_args))
        elif args.wide_variants_out:                          # (one pass gives both tables)
            id_rows, var_rows = block_wide_variants(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits)
            with open(args.wide_variants_out, "w", encoding="utf-8") as fh:
                fh.write(wide_variants_table(var_rows, *id_args, args.identity_max_edits))
        elif args.identity_out:
            id_rows = block_identity(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits)
        if args.identity_out:
            with open(args.identity_out, "w", encoding="utf-8") as fh:
                fh.write(identity_table(id_rows, *id_args, max_edits=args.identity_max_edits))
        if args.ends_out:
            e_args = id_args + (args.identity_max_edits, args.ends_max_len, args.ends_max_edits, args.ends_penalty)
            if args.end_variants_out:                         # (one pass gives both tables)
                end_rows, end_variant_rows = block_ends(ctx, loaders, read_blocks(args.tsv), *e_args, with_variants=True)
                with open(args.end_variants_out, "w", encoding="utf-8") as fh:
                    fh.write(end_variants_table(end_variant_rows, *e_args))
            else:
                end_rows = block_ends(ctx, loaders, read_blocks(args.tsv), *e_args)
            with open(args.ends_out, "w", encoding="utf-8") as fh:
                fh.write(ends_table(end_rows, *e_args))
        if args.lift_joined_out or args.lift_windows_joined_out:                              # (one pass gives every file of the lift, the joined ones and the PAF)
            a_args = dict(max_edits=args.identity_max_edits, ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            intervals = read_bed(args.lift_bed) if args.lift_bed else None
            windows = window_intervals(record_sizes(loaders, args.lift_genome), args.lift_windows) if args.lift_windows is not None else None
            got = block_lifts(ctx, loaders, read_blocks(args.tsv), args.lift_genome, *id_args, **a_args, lift=intervals if args.lift_out else None,
                              identity=([intervals] if args.lift_identity_out else []) + ([windows] if args.lift_windows_out else []),
                              joined=([intervals] if args.lift_joined_out else []) + ([windows] if args.lift_windows_joined_out else []),
                              paf=bool(args.paf_out), cs=args.paf_cs)
            files = [(args.paf_out, paf_table(got["paf"]))] if args.paf_out else []
            files += [(args.lift_out, lift_table(got["lift"], *id_args, **a_args))] if args.lift_out else []
            files += [(path, lift_identity_table(rows, *id_args, **a_args))
                      for path, rows in zip([f for f in (args.lift_identity_out, args.lift_windows_out) if f], got["identity"])]
            files += [(path, lift_joined_table(rows, *id_args, **a_args))
                      for path, rows in zip([f for f in (args.lift_joined_out, args.lift_windows_joined_out) if f], got["joined"])]
            for path, text_ in files:
                with open(path, "w", encoding="utf-8") as fh:
                    fh.write(text_)
        elif args.lift_identity_out or args.lift_windows_out:   # (one pass gives every file of the lift, and the PAF)
            a_args = dict(max_edits=args.identity_max_edits, ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            intervals = read_bed(args.lift_bed) if args.lift_bed else None
            sets = ([intervals] if args.lift_identity_out else []) + \
                ([window_intervals(record_sizes(loaders, args.lift_genome), args.lift_windows)] if args.lift_windows_out else [])
            if args.paf_out:
                paf_rows, lift_rows_, counted = block_alignments(ctx, loaders, read_blocks(args.tsv), *id_args, **a_args,
                                                                 lift=(args.lift_genome, intervals) if args.lift_out else None,
                                                                 lift_identity=(args.lift_genome, sets), cs=args.paf_cs)
                with open(args.paf_out, "w", encoding="utf-8") as fh:
                    fh.write(paf_table(paf_rows))
            else:
                counted = block_lift_identity(ctx, loaders, read_blocks(args.tsv), args.lift_genome, sets, *id_args, **a_args,
                                              lift=intervals if args.lift_out else None)
                if args.lift_out:
                    lift_rows_, counted = counted
            if args.lift_out:
                with open(args.lift_out, "w", encoding="utf-8") as fh:
                    fh.write(lift_table(lift_rows_, *id_args, **a_args))
            for path, rows in zip([f for f in (args.lift_identity_out, args.lift_windows_out) if f], counted):
                with open(path, "w", encoding="utf-8") as fh:
                    fh.write(lift_identity_table(rows, *id_args, **a_args))
        elif args.paf_out or args.lift_out:                   # (one pass gives both files)
            a_args = dict(max_edits=args.identity_max_edits, ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            intervals = read_bed(args.lift_bed) if args.lift_out else None
            if args.paf_out:
                paf_rows = block_alignments(ctx, loaders, read_blocks(args.tsv), *id_args, **a_args,
                                            lift=(args.lift_genome, intervals) if args.lift_out else None, cs=args.paf_cs, chain=bool(args.chain_out))
                if args.chain_out:                            # (one pass gives the PAF and the chain file)
                    paf_rows, chain_parts = (paf_rows[:-1] if args.lift_out else paf_rows[0]), paf_rows[-1]
                if args.lift_out:
                    paf_rows, lift_rows_ = paf_rows
                with open(args.paf_out, "w", encoding="utf-8") as fh:
                    fh.write(paf_table(paf_rows))
            else:
                lift_rows_ = block_lift(ctx, loaders, read_blocks(args.tsv), args.lift_genome, intervals, *id_args, **a_args)
            if args.lift_out:
                with open(args.lift_out, "w", encoding="utf-8") as fh:
                    fh.write(lift_table(lift_rows_, *id_args, **a_args))
        if args.chain_out:
            if chain_parts is None:                           # (beside the lift tables or alone: a pass of its own)
                chain_parts = block_chains(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits,
                                           ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            with open(args.chain_out, "w", encoding="utf-8") as fh:
                fh.write(chain_table(chain_parts))
        if args.maf_out:                                      # (a pass of its own)
            maf_parts = block_mafs(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits,
                                   ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            with open(args.maf_out, "w", encoding="utf-8") as fh:
                fh.write(maf_table(maf_parts))
        if args.multi_maf_out:                                # (a pass of its own)
            multi_parts = block_multi_mafs(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits,
                                           ends=(args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None)
            with open(args.multi_maf_out, "w", encoding="utf-8") as fh:
                fh.write(multi_maf_table(multi_parts))
        if args.conservation_out:                             # (a pass of its own)
            c_ends = (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None
            conserved = block_conservation(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits, ends=c_ends)
            for path, table in ((args.conservation_out, conservation_bed), (args.conservation_stats_out, conservation_table)):
                with open(path, "w", encoding="utf-8") as fh:
                    fh.write(table(*conserved, *id_args, max_edits=args.identity_max_edits, ends=c_ends))
        if args.variant_sites_out:                            # (a pass of its own)
            v_ends = (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None
            sites = block_variant_sites(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits, ends=v_ends)
            with open(args.variant_sites_out, "w", encoding="utf-8") as fh:
                fh.write(variant_sites_table(*sites, *id_args, max_edits=args.identity_max_edits, ends=v_ends))
        if args.profile_out:                                  # (a pass of its own)
            f_ends = (args.ends_max_len, args.ends_max_edits, args.ends_penalty) if args.ends_out else None
            profile = block_consensus(ctx, loaders, read_blocks(args.tsv), *id_args, max_edits=args.identity_max_edits, ends=f_ends)
            with open(args.profile_out, "w", encoding="utf-8") as fh:
                fh.write(profile_table(*profile[:3], *id_args, max_edits=args.identity_max_edits, ends=f_ends))
            with open(args.consensus_out, "w", encoding="utf-8") as fh:
                fh.write(consensus_fasta(*profile, consensus_reference_bases(loaders, profile[0], profile[3])))
    finally:
        ctx.close()
    if args.divergence_out:
        with open(args.divergence_out, "w", encoding="utf-8") as fh:
            fh.write(text)
    else:
        print(text, end="")
    return 0

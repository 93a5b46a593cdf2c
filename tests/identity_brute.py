"""Brute forces for the block identity (docs/design/04_16_block_identity.md), straight from the definitions: dictionaries for the
anchors, the full (dx + 1) x (dy + 1) table for the edit distance (one numpy row at a time), integer arithmetic for the file.  No GPU,
nothing of ntsynt_amd.assess.block_identity."""
from collections import Counter

import numpy as np

CANDIDATE, BACKWARD, LONG, OFFBAND = 0, 1, 2, 3
NOT_CANDIDATE, PASSED, OVERBAND, INVALID = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NO_MATE = 0xFFFFFFFF
COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}                 # A <-> T, C <-> G (ASCII)
COLUMNS = ("block_id", "genome_a", "genome_b", "orientation", "length_a", "length_b", "anchors", "segments", "aligned", "aligned_a", "aligned_b",
           "edits", "identity", "covered_a", "covered_b", "backward", "long", "offband", "invalid", "overband")


def kind_of(dx, dy, band, max_len):
    if dy <= 0:
        return BACKWARD
    if max(dx, dy) > max_len:
        return LONG
    if abs(dy - dx) > band:
        return OFFBAND
    return CANDIDATE


def brute_segments(recs_a, recs_b, mate, len_b, flip, k, band, max_len):
    """recs: (h0, iv, off) triples of each genome.  Returns (segments as (iv_a, x, dx, y_lo, dy, kind) in (iv_a, x) order, anchors per
    interval of A)"""
    count_a, count_b = Counter(h for h, _, _ in recs_a), Counter(h for h, _, _ in recs_b)
    where_b = {h: (iv, off) for h, iv, off in recs_b if count_b[h] == 1}
    anchors = {}
    for h, iv, off in recs_a:
        if count_a[h] != 1 or h not in where_b or mate[iv] == NO_MATE or where_b[h][0] != mate[iv]:
            continue
        off_b = where_b[h][1]
        anchors.setdefault(iv, []).append((off, len_b[iv] - k - off_b if flip[iv] else off_b))
    per_iv = [len(anchors.get(iv, ())) for iv in range(len(mate))]
    segs = []
    for iv in sorted(anchors):
        pts = sorted(anchors[iv])
        for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
            segs.append((iv, x0, x1 - x0, y0, y1 - y0, kind_of(x1 - x0, y1 - y0, band, max_len)))
    return segs, per_iv


def levenshtein(a, b):
    "unit-cost edit distance of two uint8 arrays: the whole table, a row at a time"
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    if a.size == b.size:
        differing = int((a != b).sum())
        if differing <= 1:                                    # (exact: D <= the Hamming distance, and D = 0 only for equal strings)
            return differing
    ramp = np.arange(b.size + 1, dtype=np.int64)
    row = ramp.copy()
    for i in range(a.size):
        best = np.empty_like(row)
        best[0] = i + 1
        np.minimum(row[1:] + 1, row[:-1] + (b != a[i]), out=best[1:])
        row = np.minimum.accumulate(best - ramp) + ramp      # row[j] = min over j' <= j of best[j'] + (j - j'): the steps along the row
    return int(row[-1])


def revcomp(seq):
    "reverse complement of an ASCII uint8 array; a letter that is not A, C, G, T stays what it is"
    table = np.arange(256, dtype=np.uint8)
    for x, y in COMPLEMENT.items():
        table[x] = y
    return table[np.asarray(seq, dtype=np.uint8)[::-1]]


def strings_of(seq_a, seq_b, iv_a, iv_b, flip, seg):
    """the two strings of a segment.  seq: a genome's concatenated records (ASCII), iv: (absolute start, length) of the clipped
    interval"""
    _, x, dx, y_lo, dy, _ = seg
    a0, la = iv_a
    b0, lb = iv_b
    assert 0 <= x and x + dx <= la and 0 <= y_lo and y_lo + dy <= lb
    a = seq_a[a0 + x:a0 + x + dx]
    b = revcomp(seq_b[b0 + lb - y_lo - dy:b0 + lb - y_lo]) if flip else seq_b[b0 + y_lo:b0 + y_lo + dy]
    return a, b


def brute_edit(seq_a, seq_b, ivs_a, ivs_b, flip, segs, band):
    "(per-segment results, per-interval dicts) of nts_edit_segments; ivs: (absolute start, length) per interval of A and of its mate"
    valid = np.zeros(256, dtype=bool)
    valid[list(COMPLEMENT)] = True
    dist = []
    per_iv = [dict(aligned_a=0, aligned_b=0, edits=0, segments=0, aligned=0, backward=0, too_long=0, offband=0, invalid=0, overband=0)
              for _ in ivs_a]
    for seg in segs:
        iv, _, dx, _, dy, kind = seg
        row = per_iv[iv]
        row["segments"] += 1
        if kind != CANDIDATE:
            name = {BACKWARD: "backward", LONG: "too_long", OFFBAND: "offband"}.get(kind)
            if name:
                row[name] += 1
            dist.append(PASSED if name else NOT_CANDIDATE)
            continue
        a, b = strings_of(seq_a, seq_b, ivs_a[iv], ivs_b[iv], flip[iv], seg)
        if not (valid[a].all() and valid[b].all()):
            row["invalid"] += 1
            dist.append(INVALID)
            continue
        d = levenshtein(a, b)
        if (d + abs(dy - dx)) // 2 > band:
            row["overband"] += 1
            dist.append(OVERBAND)
            continue
        row["aligned"] += 1
        row["aligned_a"] += dx
        row["aligned_b"] += dy
        row["edits"] += d
        dist.append(d)
    return dist, per_iv


def format_row(r):
    "one line of the file from a dict of integers and names (the definitions' arithmetic)"
    m = max(r["aligned_a"], r["aligned_b"])
    if m == 0:
        identity = "."
    else:
        v = (1000000 * (m - r["edits"])) // m
        identity = f"{v // 1000000}.{v % 1000000:06d}"

    def covered(x, length):
        if length == 0:
            return "."
        v = (1000 * x) // length
        return f"{v // 10}.{v % 10}"
    f = dict(r, identity=identity, covered_a=covered(r["aligned_a"], r["length_a"]), covered_b=covered(r["aligned_b"], r["length_b"]))
    return "\t".join(str(f[c]) for c in COLUMNS)


def block_key(b):
    return (0, int(b), "") if b.lstrip("-").isdigit() else (1, 0, b)


def brute_file(table, genomes, hash_all, k, rate, band, max_len):
    """the whole file.  table: rows with .block_id .genome .contig .start .end .strand in file order; genomes: {name: {contig: ASCII
    uint8 array}}; hash_all(bytes, k) -> (positions, h0) of every valid k-mer.  Returns (text, facts): facts[(block, genome_a,
    genome_b)] = (row dict, [(segment tuple, result)])"""
    limit = ((1 << 64) - 1) // rate
    lines_of = {}
    for i, r in enumerate(table):
        lines_of.setdefault(r.genome, []).append(i)
    clipped = {}
    for i, r in enumerate(table):
        n = genomes[r.genome][r.contig].size
        a, b = min(max(r.start, 0), n), min(max(r.end, 0), n)
        clipped[i] = (a, max(b - a, 0))
    hashed = {}
    recs = {}                                                 # genome -> [(h0, line, off)] over ALL its lines
    for name, lines in lines_of.items():
        out = []
        for i in lines:
            r = table[i]
            if (name, r.contig) not in hashed:
                pos, h0 = hash_all(genomes[name][r.contig].tobytes(), k)
                hashed[(name, r.contig)] = (np.asarray(pos, dtype=np.int64), np.asarray(h0, dtype=np.uint64))
            pos, h0 = hashed[(name, r.contig)]
            a, n = clipped[i]
            keep = (pos >= a) & (pos + k <= a + n) & (h0 <= np.uint64(limit))
            out += [(int(h), i, int(p) - a) for p, h in zip(pos[keep], h0[keep])]
        recs[name] = out
    counts = {name: Counter(h for h, _, _ in out) for name, out in recs.items()}
    once = {name: {h: (i, off) for h, i, off in out if counts[name][h] == 1} for name, out in recs.items()}
    by_id = {}
    for i, r in enumerate(table):
        by_id.setdefault(r.block_id, []).append(i)
    text, facts = ["\t".join(COLUMNS)], {}
    for b in sorted(by_id, key=block_key):
        lines = by_id[b]
        for xi in range(len(lines)):
            for yi in range(xi + 1, len(lines)):
                la, lb = lines[xi], lines[yi]
                ra, rb = table[la], table[lb]
                flip = ra.strand != rb.strand
                (a0, len_a), (b0, len_b) = clipped[la], clipped[lb]
                pts = []
                for h, (i, off) in once[ra.genome].items():
                    if i == la and once[rb.genome].get(h, (None, 0))[0] == lb and (ra.genome != rb.genome or la != lb):
                        off_b = once[rb.genome][h][1]
                        pts.append((off, len_b - k - off_b if flip else off_b))
                pts.sort()
                segs = [(0, x0, x1 - x0, y0, y1 - y0, kind_of(x1 - x0, y1 - y0, band, max_len)) for (x0, y0), (x1, y1) in zip(pts, pts[1:])]
                seq_a, seq_b = genomes[ra.genome][ra.contig], genomes[rb.genome][rb.contig]
                dist, per = brute_edit(seq_a, seq_b, [(a0, len_a)], [(b0, len_b)], [flip], segs, band)
                p = per[0]
                row = dict(block_id=b, genome_a=ra.genome, genome_b=rb.genome, orientation="-" if flip else "+", length_a=len_a, length_b=len_b,
                           anchors=len(pts), segments=p["segments"], aligned=p["aligned"], aligned_a=p["aligned_a"], aligned_b=p["aligned_b"],
                           edits=p["edits"], backward=p["backward"], long=p["too_long"], offband=p["offband"], invalid=p["invalid"],
                           overband=p["overband"])
                text.append(format_row(row))
                facts[(b, ra.genome, rb.genome)] = (row, list(zip(segs, dist)))
    text.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}")
    return "\n".join(text) + "\n", facts

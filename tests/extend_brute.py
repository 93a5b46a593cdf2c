"""Brute force for the free-end extension (docs/design/04_20_block_ends.md), the definition literally: both strings cut before their
first base that is not A, C, G or T, the full unrestricted unit-cost edit table T (one numpy row at a time, every row kept), the cells
with T <= E, S = i + j - P T, and the tie order: the least T, then the least d = j - i.  No GPU, nothing of ntsynt_amd."""
import numpy as np

COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}                 # A <-> T, C <-> G (ASCII)
A_BACKWARDS, B_BACKWARDS, B_COMPLEMENT = 1, 2, 4


def _valid():
    ok = np.zeros(256, dtype=bool)
    ok[list(COMPLEMENT)] = True
    return ok


VALID = _valid()


def complement(seq):
    "every base complemented, the order kept; a letter that is not A, C, G, T stays what it is"
    table = np.arange(256, dtype=np.uint8)
    for x, y in COMPLEMENT.items():
        table[x] = y
    return table[np.asarray(seq, dtype=np.uint8)]


def read_string(record, pos, n, backwards, comp=False):
    "the n bases of an ASCII record from position pos, forwards or backwards, complemented or not; nothing outside the record is read"
    pos, n = int(pos), int(n)
    if n == 0:
        assert 0 <= pos <= record.size
        return np.zeros(0, dtype=np.uint8)
    if backwards:
        assert n <= pos + 1 <= record.size, (pos, n, record.size)
        s = record[pos - n + 1:pos + 1][::-1]
    else:
        assert pos + n <= record.size, (pos, n, record.size)
        s = record[pos:pos + n]
    return complement(s) if comp else s.copy()


def cut(s):
    "the number of bases in front of the first one that is not A, C, G or T"
    bad = np.flatnonzero(~VALID[np.asarray(s, dtype=np.uint8)])
    return int(bad[0]) if bad.size else int(np.asarray(s).size)


def table(a, b):
    "T[i][j] = the unit-cost edit distance of a[:i] and b[:j], all of it, int32"
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    ramp = np.arange(b.size + 1, dtype=np.int32)
    t = np.empty((a.size + 1, b.size + 1), dtype=np.int32)
    t[0] = ramp
    best = np.empty(b.size + 1, dtype=np.int32)
    for i in range(a.size):
        row = t[i]
        best[0] = i + 1
        np.minimum(row[1:] + 1, row[:-1] + (b != a[i]), out=best[1:])
        t[i + 1] = np.minimum.accumulate(best - ramp) + ramp  # t[i+1][j] = min over j' <= j of best[j'] + (j - j'): the steps along the row
    return t


def extend_brute(a, b, penalty, max_edits):
    """a, b: the two strings as read (oriented, complemented), ASCII.  Returns ((ext_a, ext_b, edits, valid_a, valid_b), the number of
    cells that attain the largest S)"""
    assert 3 <= penalty <= 255 and 1 <= max_edits <= 1023
    nv, mv = cut(a), cut(b)
    t = table(np.asarray(a)[:nv], np.asarray(b)[:mv])
    i = np.arange(nv + 1, dtype=np.int64)[:, None]
    j = np.arange(mv + 1, dtype=np.int64)[None, :]
    allowed = t <= max_edits
    s = np.where(allowed, i + j - penalty * t.astype(np.int64), np.iinfo(np.int64).min)
    top = s.max()                                             # (cell (0, 0) is always allowed)
    cells = np.argwhere(s == top)
    order = sorted((int(t[ci, cj]), int(cj) - int(ci), int(ci), int(cj)) for ci, cj in cells)
    edits, _, bi, bj = order[0]
    return (bi, bj, edits, nv, mv), len(order)


def task_strings(records_a, records_b, task):
    "the two strings of a task (rec_a, pos_a, n, rec_b, pos_b, m, flags) over two genomes' lists of ASCII records"
    rec_a, pos_a, n, rec_b, pos_b, m, flags = (int(x) for x in task)
    return (read_string(records_a[rec_a], pos_a, n, bool(flags & A_BACKWARDS)),
            read_string(records_b[rec_b], pos_b, m, bool(flags & B_BACKWARDS), bool(flags & B_COMPLEMENT)))


# ---- the block ends file (ntsynt_amd/assess.py block_ends) from the identity brute force's segments: no GPU, nothing of assess

ENDS_COLUMNS = ("block_id", "genome_a", "contig_a", "start_a", "end_a", "genome_b", "contig_b", "start_b", "end_b", "orientation", "left_a", "left_b",
                "left_edits", "left_stop", "right_a", "right_b", "right_edits", "right_stop", "ext_start_a", "ext_end_a", "ext_start_b", "ext_end_b")
INVALID_RESULT = 0xFFFFFFFC                                   # a per-segment result below this is a distance


def revcomp(seq):
    return complement(seq)[::-1]


def stop_reason(result, asked_a, asked_b, max_len, max_edits):
    "the definition's two lists of precedence"
    ext_a, ext_b, edits, valid_a, valid_b = result

    def kind(valid, asked):
        if valid < asked:
            return "invalid"
        return "max_len" if asked == max_len else "record"
    if ext_a == valid_a:
        return kind(valid_a, asked_a)
    if ext_b == valid_b:
        return kind(valid_b, asked_b)
    return "max_edits" if edits == max_edits else "break"


def pair_ends(seq_a, seq_b, iv_a, iv_b, flip, results, max_len, max_edits, penalty):
    """the flanks of one pair.  seq_*: the two whole records (ASCII), iv_*: (start, length) of the clipped intervals, results: [(segment
    tuple, final result)] in (x) order.  A flipped pair is worked in the frame of the WHOLE record's reverse complement, where B runs
    like A, and only the final coordinates are mapped back.  Returns None without an aligned segment, else a dict of the twelve
    columns behind `orientation`."""
    aligned = [seg for seg, d in results if d < INVALID_RESULT]
    if not aligned:
        return None
    (_, x_l, _, y_l, _, _), (_, x, dx, y, dy, _) = aligned[0], aligned[-1]
    x_r, y_r = x + dx, y + dy
    frame_b = revcomp(seq_b) if flip else seq_b
    start_a, start_b = iv_a[0], (seq_b.size - iv_b[0] - iv_b[1]) if flip else iv_b[0]
    out = {}
    # right: forwards from the right end point
    pa, pb = start_a + x_r, start_b + y_r
    n, m = min(max_len, seq_a.size - pa), min(max_len, frame_b.size - pb)
    right, _ = extend_brute(seq_a[pa:pa + n], frame_b[pb:pb + m], penalty, max_edits)
    out["right_stop"] = stop_reason(right, n, m, max_len, max_edits)
    # left: backwards from the base in front of the left end point
    qa, qb = start_a + x_l, start_b + y_l
    n, m = min(max_len, qa), min(max_len, qb)
    left, _ = extend_brute(seq_a[qa - n:qa][::-1], frame_b[qb - m:qb][::-1], penalty, max_edits)
    out["left_stop"] = stop_reason(left, n, m, max_len, max_edits)
    out.update(left_a=left[0], left_b=left[1], left_edits=left[2], right_a=right[0], right_b=right[1], right_edits=right[2])
    out["ext_start_a"], out["ext_end_a"] = qa - left[0], pa + right[0]
    lo, hi = qb - left[1], pb + right[1]                      # in B's frame
    out["ext_start_b"], out["ext_end_b"] = (seq_b.size - hi, seq_b.size - lo) if flip else (lo, hi)
    return out


def ends_file(table, genomes, facts, k, rate, band, max_len, max_edits, ends_max_len, ends_max_edits, ends_penalty):
    """the whole file.  table: the block lines; genomes: {name: {contig: ASCII uint8 array}}; facts: identity_brute.brute_file's (or
    wide_brute.brute_file_wide's) facts for (k, rate, band, max_len, max_edits), whose order is the file's.  Returns (text, {key: the
    pair's dict or None})"""
    line_of = {(r.block_id, r.genome): r for r in table}
    lines, found = ["\t".join(ENDS_COLUMNS)], {}
    for (b, name_a, name_b), (row, results) in facts.items():
        ra, rb = line_of[(b, name_a)], line_of[(b, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        clip = lambda r, n: (min(max(r.start, 0), n), max(min(max(r.end, 0), n) - min(max(r.start, 0), n), 0))      # noqa: E731
        iv_a, iv_b = clip(ra, seq_a.size), clip(rb, seq_b.size)
        flip = ra.strand != rb.strand
        assert row["orientation"] == ("-" if flip else "+")
        ends = pair_ends(seq_a, seq_b, iv_a, iv_b, flip, results, ends_max_len, ends_max_edits, ends_penalty)
        found[(b, name_a, name_b)] = ends
        head = [b, name_a, ra.contig, iv_a[0], iv_a[0] + iv_a[1], name_b, rb.contig, iv_b[0], iv_b[0] + iv_b[1], "-" if flip else "+"]
        lines.append("\t".join(str(x) for x in head + [ends[c] if ends else "." for c in ENDS_COLUMNS[10:]]))
    lines.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}, ends_max_len {ends_max_len}, "
                 f"ends_max_edits {ends_max_edits}, ends_penalty {ends_penalty}")
    return "\n".join(lines) + "\n", found

"""Brute force for the block end variants (docs/design/04_21_block_end_variants.md): the flanks' strings taken in the frame of the WHOLE
record's reverse complement for a flipped pair, as tests/extend_brute.pair_ends takes them, the extension by extend_brute, the canonical
script of the two extended strings by variants_brute.script, its events by variants_brute.events, and the events' forward record
coordinates worked out here from the frame's intervals.  No GPU, nothing of ntsynt_amd.assess."""
from tests import extend_brute as X
from tests import variants_brute as V

COLUMNS = ("block_id", "genome_a", "contig_a", "pos_a", "genome_b", "contig_b", "pos_b", "orientation", "flank", "type", "length", "seq_a", "seq_b")


def flank_events(a, b, penalty, max_edits):
    "((ext_a, ext_b, edits, ...), [(type, p0, q0, bases of A, bases of B)]) of two strings as read outwards"
    res, _ = X.extend_brute(a, b, penalty, max_edits)
    a1, b1 = a[:res[0]], b[:res[1]]
    ops = V.script(a1, b1)
    assert len(ops) == res[2]
    return res, V.events(ops, a1, b1)


def pair_events(seq_a, seq_b, iv_a, iv_b, flip, results, max_len, max_edits, penalty):
    """the events of one pair's two flanks: [(flank, pos_a, pos_b, type, length, seq_a, seq_b)], left before right, each ascending
    along A, and {flank: edits}.  Arguments as extend_brute.pair_ends."""
    aligned = [seg for seg, d in results if d < X.INVALID_RESULT]
    if not aligned:
        return [], {}
    (_, x_l, _, y_l, _, _), (_, x, dx, y, dy, _) = aligned[0], aligned[-1]
    x_r, y_r = x + dx, y + dy
    frame_b = X.revcomp(seq_b) if flip else seq_b
    start_a, start_b = iv_a[0], (seq_b.size - iv_b[0] - iv_b[1]) if flip else iv_b[0]

    def forward_b(lo, hi):
        "the start in B's record of the frame's interval [lo, hi)"
        return seq_b.size - hi if flip else lo
    out, edits = [], {}
    # left: backwards from the base in front of the left end point; offset p of the string is frame position qa - 1 - p
    qa, qb = start_a + x_l, start_b + y_l
    n, m = min(max_len, qa), min(max_len, qb)
    res, events = flank_events(seq_a[qa - n:qa][::-1], frame_b[qb - m:qb][::-1], penalty, max_edits)
    edits["left"] = res[2]
    for kind, p0, q0, bases_a, bases_b in events[::-1]:
        out.append(("left", qa - p0 - len(bases_a), forward_b(qb - q0 - len(bases_b), qb - q0), kind, max(len(bases_a), len(bases_b)),
                    bases_a[::-1] or "-", bases_b[::-1] or "-"))
    # right: forwards from the right end point
    pa, pb = start_a + x_r, start_b + y_r
    n, m = min(max_len, seq_a.size - pa), min(max_len, frame_b.size - pb)
    res, events = flank_events(seq_a[pa:pa + n], frame_b[pb:pb + m], penalty, max_edits)
    edits["right"] = res[2]
    for kind, p0, q0, bases_a, bases_b in events:
        out.append(("right", pa + p0, forward_b(pb + q0, pb + q0 + len(bases_b)), kind, max(len(bases_a), len(bases_b)), bases_a or "-", bases_b or "-"))
    return out, edits


def end_variants_file(table, genomes, facts, k, rate, band, max_len, max_edits, ends_max_len, ends_max_edits, ends_penalty):
    """the whole file.  Arguments as extend_brute.ends_file.  Returns (text, {key: ([event tuples], {flank: edits})})"""
    line_of = {(r.block_id, r.genome): r for r in table}
    lines, found = ["\t".join(COLUMNS)], {}
    for (b, name_a, name_b), (row, results) in facts.items():
        ra, rb = line_of[(b, name_a)], line_of[(b, name_b)]
        seq_a, seq_b = genomes[name_a][ra.contig], genomes[name_b][rb.contig]
        clip = lambda r, n: (min(max(r.start, 0), n), max(min(max(r.end, 0), n) - min(max(r.start, 0), n), 0))      # noqa: E731
        flip = ra.strand != rb.strand
        events, edits = pair_events(seq_a, seq_b, clip(ra, seq_a.size), clip(rb, seq_b.size), flip, results, ends_max_len, ends_max_edits, ends_penalty)
        found[(b, name_a, name_b)] = (events, edits)
        for flank, pos_a, pos_b, kind, length, bases_a, bases_b in events:
            lines.append("\t".join(str(v) for v in (b, name_a, ra.contig, pos_a, name_b, rb.contig, pos_b, "-" if flip else "+", flank, kind, length,
                                                    bases_a, bases_b)))
    lines.append(f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}, ends_max_len {ends_max_len}, "
                 f"ends_max_edits {ends_max_edits}, ends_penalty {ends_penalty}")
    return "\n".join(lines) + "\n", found

"""The definition of docs/design/04_31_block_conservation.md restated on the CPU, base by base: a dictionary of per-base triples filled
by walking every chain, then run-length encoded.  Plain Python over lists and dictionaries; it shares no code with ntsynt_amd/assess.py
and reads nothing of it.  Used by tests/test_gpu_cigar_depth.py, tests/test_gpu_cigar_depth_order.py, tests/test_conservation_host.py
and tests/test_gpu_block_conservation.py."""

I, D, EQ, X = 1, 2, 7, 8


def triples(chains):
    "chains: (group, t0, entries) each.  Returns {(group, base): [aligned, match, gap]} of every base some chain covers"
    seen = {}
    for group, t0, entries in chains:
        p = t0
        for v in entries:
            code, size = v & 15, v >> 4
            if code == I:
                continue
            assert code in (D, EQ, X), code
            for q in range(p, p + size):
                t = seen.setdefault((group, q), [0, 0, 0])
                t[0] += 1
                t[1] += code == EQ
                t[2] += code == D
            p += size
    return seen


def segments(chains, n_groups):
    """What Context.cigar_depth returns, as lists: (segs, seg_first) with segs = (start, end, group, aligned, match, gap) tuples ascending
    by (group, start): the maximal runs of consecutive bases of one group with one triple"""
    seen = triples(chains)
    segs = []
    for group, p in sorted(seen):
        t = tuple(seen[(group, p)])
        if segs and segs[-1][2] == group and segs[-1][1] == p and segs[-1][3:] == t:
            segs[-1] = (segs[-1][0], p + 1) + segs[-1][2:]
        else:
            segs.append((p, p + 1, group) + t)
    first = [sum(1 for s in segs if s[2] < g) for g in range(n_groups + 1)]
    return segs, first


def summary(segs, n_groups, rows):
    "per group {covered, core, conserved, by_aligned[1 .. rows], by_match[0 .. rows]}, counted base by base.  rows[g]: the group's rows"
    out = [{"covered": 0, "core": 0, "conserved": 0, "by_aligned": [0] * rows[g], "by_match": [0] * (rows[g] + 1)} for g in range(n_groups)]
    for start, end, group, aligned, match, gap in segs:
        s = out[group]
        for _ in range(start, end):
            s["covered"] += 1
            s["by_aligned"][aligned - 1] += 1
            if aligned == rows[group]:
                s["core"] += 1
                s["by_match"][match] += 1
                s["conserved"] += match == rows[group]
    return out


def parameters(k, rate, band, max_len, max_edits, ends):
    text = f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}"
    if ends is not None:
        text += f", ends_max_len {ends[0]}, ends_max_edits {ends[1]}, ends_penalty {ends[2]}"
    return text


def bed_text(groups, segs, params):
    "groups: per group (block_id, genome, contig, start, end, rows).  The text of <prefix>.block_conservation.bed"
    lines = [parameters(*params)]
    for start, end, group, aligned, match, gap in segs:
        block_id, genome, contig, _, _, rows = groups[group]
        lines.append("\t".join(str(v) for v in (contig, start, end, block_id, genome, rows, aligned, match, aligned - match - gap, gap)))
    return "\n".join(lines) + "\n"


def table_text(groups, segs, params):
    "the text of <prefix>.block_conservation.tsv"
    names = ("block_id", "genome", "contig", "start", "end", "rows", "covered", "core", "conserved", "by_aligned", "by_match")
    lines = ["\t".join(names)]
    for g, s in zip(groups, summary(segs, len(groups), [g[5] for g in groups])):
        lines.append("\t".join([str(v) for v in g] + [str(s["covered"]), str(s["core"]), str(s["conserved"]), ",".join(str(v) for v in s["by_aligned"]),
                                                      ",".join(str(v) for v in s["by_match"])]))
    lines.append(parameters(*params))
    return "\n".join(lines) + "\n"

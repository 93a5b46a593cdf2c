"""The definitions of docs/design/04_33_block_consensus.md restated on the CPU, column by column: every chain is walked over its
columns and fills a dictionary keyed by (group, pos, sub) with tallies, the covering chains of a column are counted by a loop over its
group's chains, the call is decided by the rule as it is written.  Plain Python over lists and dictionaries; it shares no code with
ntsynt_amd/assess.py and reads nothing of it.  Used by tests/test_gpu_cigar_profile.py, tests/test_gpu_cigar_profile_order.py,
tests/test_consensus_host.py and tests/test_gpu_block_consensus.py."""

I, D, EQ, X = 1, 2, 7, 8
REF = 0xFFFFFFFF
SYMBOLS = "ACGTN-"
FIELDS = ("pos", "group", "sub", "aligned", "match", "gap", "n", "ref", "call")


def symbol_of(byte):
    "0 .. 3 for A C G T, 4 (N) for every other byte"
    return "ACGT".index(chr(byte)) if chr(byte) in "ACGT" else 4


def byte_counts(entries):
    "(ref bytes, alt bytes) of one chain: its X + D and its X + I lengths"
    return (sum(v >> 4 for v in entries if v & 15 in (X, D)), sum(v >> 4 for v in entries if v & 15 in (X, I)))


def decide(tally, own):
    "tally: six counts in the order A C G T N -; own: the reference's symbol.  The symbol of the largest tally, ties by the rule"
    most = max(tally)
    if tally[own] == most:
        return own
    return next(s for s in range(6) if tally[s] == most)


def columns(chains, refs, alts, n_groups):
    """chains: (group, t0, entries) each; refs[c], alts[c]: chain c's ref and alt bytes.  What Context.cigar_profile returns, as lists:
    (cols, col_first) with cols = (pos, group, sub, aligned, match, gap, (nA, nC, nG, nT, nN), ref, call) tuples in the definition's
    order, ref and call as one-character strings"""
    ends = [t0 + sum(v >> 4 for v in entries if v & 15 != I) for _, t0, entries in chains]
    seen = {}                                                 # (group, pos, sub) -> [n[0..4], gap events, the ref byte of the smallest chain]
    for (group, t0, entries), ref, alt in zip(chains, refs, alts):
        p, r, a = t0, 0, 0
        for v in entries:
            code, size = v & 15, v >> 4
            for j in range(size):
                if code == X:
                    mine = seen.setdefault((group, p, REF), [[0] * 5, 0, ref[r]])
                    mine[0][symbol_of(alt[a])] += 1
                    p, r, a = p + 1, r + 1, a + 1
                elif code == D:
                    seen.setdefault((group, p, REF), [[0] * 5, 0, ref[r]])[1] += 1
                    p, r = p + 1, r + 1
                elif code == I:
                    seen.setdefault((group, p, j), [[0] * 5, 0, ord("-")])[0][symbol_of(alt[a])] += 1
                    a += 1
                else:
                    assert code == EQ, code
                    p += 1
        assert (r, a) == (len(ref), len(alt)), (r, a, len(ref), len(alt))
    out = []
    for group, pos, sub in sorted(seen):
        n, gone, ref = seen[(group, pos, sub)]
        aligned = sum(1 for c, (g, t0, _) in enumerate(chains) if g == group and t0 <= pos < ends[c])
        if sub == REF:
            match, gap = aligned - gone - sum(n), gone
            own = symbol_of(ref)
            tally = list(n) + [gap]
            tally[own] += match + 1
        else:
            match, gap = 0, aligned - sum(n)
            own = 5
            tally = list(n) + [gap + 1]
        assert sum(tally) == aligned + 1 and match >= 0 and gap >= 0, (group, pos, sub)
        out.append((pos, group, sub, aligned, match, gap, tuple(n), chr(ref), SYMBOLS[decide(tally, own)]))
    return out, [sum(1 for c in out if c[1] < g) for g in range(n_groups + 1)]


def as_tuples(cols):
    "a CIG_PROFILE_COL_DTYPE array as columns' tuples"
    return [(int(c["pos"]), int(c["group"]), int(c["sub"]), int(c["aligned"]), int(c["match"]), int(c["gap"]), tuple(int(x) for x in c["n"]),
             chr(int(c["ref"])), chr(int(c["call"]))) for c in cols]


def tallies(col):
    "the six tallies of one column's tuple with the reference row counted in"
    pos, group, sub, aligned, match, gap, n, ref, call = col
    tally = list(n) + [gap]
    if sub == REF:
        tally[symbol_of(ord(ref))] += match + 1
    else:
        tally[5] += 1
    return tally


def extents(chains, n_groups):
    "per group (R0, R1): the smallest t0 and the largest t1 of its chains, None for a group without chains"
    out = [None] * n_groups
    for group, t0, entries in chains:
        t1 = t0 + sum(v >> 4 for v in entries if v & 15 != I)
        out[group] = (t0, t1) if out[group] is None else (min(out[group][0], t0), max(out[group][1], t1))
    return out


def consensus(cols, group, extent, bases):
    "the consensus of one group, a base-by-base walk: bases = the reference's letters of [R0, R1) as a str"
    mine = {(pos, sub): call for pos, g, sub, _, _, _, _, _, call in cols if g == group}
    out = []
    for p in range(extent[0], extent[1]):
        j = 0
        while (p, j) in mine:                                 # the slot in front of base p
            if mine[(p, j)] != "-":
                out.append(mine[(p, j)])
            j += 1
        call = mine.get((p, REF), bases[p - extent[0]])
        if call != "-":
            out.append(call)
    return "".join(out)


def parameters(k, rate, band, max_len, max_edits, ends):
    text = f"# k {k}, rate {rate}, band {band}, max_len {max_len}, max_edits {max_edits}"
    if ends is not None:
        text += f", ends_max_len {ends[0]}, ends_max_edits {ends[1]}, ends_penalty {ends[2]}"
    return text


def table_text(groups, cols, params):
    "groups: per group (block_id, genome, contig, start, end, rows).  The text of <prefix>.block_profile.tsv"
    lines = ["\t".join(("contig", "pos", "sub", "block_id", "genome", "rows", "depth", "ref", "A", "C", "G", "T", "N", "gap", "call"))]
    for col in cols:
        pos, group, sub, aligned, _, _, _, ref, call = col
        block_id, genome, contig, _, _, rows = groups[group]
        lines.append("\t".join(str(v) for v in [contig, pos, "." if sub == REF else sub, block_id, genome, rows, aligned + 1, ref] + tallies(col) + [call]))
    lines.append(parameters(*params))
    return "\n".join(lines) + "\n"


def fasta_text(groups, cols, group_extents, bases):
    "bases[g]: the reference's letters of group g's [R0, R1), a str.  The text of <prefix>.block_consensus.fa"
    lines = []
    for g, (extent, (block_id, genome, contig, _, _, rows)) in enumerate(zip(group_extents, groups)):
        if extent is None:
            continue
        mine = [c for c in cols if c[1] == g]
        lines.append(f">block_{block_id} {genome}.{contig}:{extent[0]}-{extent[1]} rows={rows} columns={len(mine)} "
                     f"changed={sum(1 for c in mine if c[8] != c[7])}")
        lines.append(consensus(cols, g, extent, bases[g]))
    return "".join(line + "\n" for line in lines)
